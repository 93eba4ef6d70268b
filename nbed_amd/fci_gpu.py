"""Determinant FCI on the device: Knowles-Handy sigma builds around one ``nbx_gemm`` and a restarted Davidson iteration.

The reference runs PySCF's ``fci.FCI`` on the embedded SCF object (nbed/driver.py:1044-1102).  ``nbed_amd.fci`` stands in
for it with a dense diagonalisation on the host, up to 16 spin orbitals.  This module is the solver for what lies
above: 10^6 - 10^7 determinants on the MI355X.

* The Hamiltonian is the ``(constant, one_body (2,n,n), two_body (3,n,n,n,n))`` of
  ``HamiltonianBuilder.build_spatial_device()``; it stays on the device and no (2n)^4 tensor is formed.
* A determinant is (alpha string, beta string); a string is an n-bit mask, ranked lexicographically by its ascending
  list of occupied orbitals (the order of ``itertools.combinations``, which is also the order in which
  ``fci.ground_state`` lists its determinants).  The CI vector is row-major ``(Na, Nb)``.  The implied operator order
  is all alpha creators before all beta creators -- ``fci.ground_state`` interleaves them, so the two vectors differ by
  a sign per determinant (``interleave_signs``).
* With E_ps = a+_p a_s:  a+_p a+_q a_r a_s = E_ps E_qr - delta_qs E_pr, so H = const + sum_g k_g E_g +
  sum_{g g'} G[g,g'] E_g E_g' over the 2n^2 same-spin generators, and a sigma is
  gather D[g,K] = <K|E_g|c> -> E = [G | k] [D ; c] (matrix cores) -> sigma_I = const c_I + sum <I|E_g|K> E[g,K],
  the last a gather per output element in a fixed order: a sigma is bit-reproducible for a given plan.
* K runs over chunks of whole alpha rows, so D and E never hold more determinants than the memory plan gives them.
* The same gather gives the densities: D_b D_c^T holds <b| E_g E_g' |c>, <b| E_g |c> and <b|c>, and an index map makes
  the spin-resolved 1- and 2-particle (transition) density matrices of it (``RdmBuilder``, ``rdm1``, ``rdm12`` and the
  methods of ``FCIGpuResult``; csrc/fci_rdm.hip).

A start vector of pure spin symmetry keeps the iteration in that symmetry when the integrals are spin-restricted, as
PySCF's solver does: from a closed-shell determinant the result is the lowest SINGLET, even where a state of another
spin lies below it in the (n_alpha, n_beta) sector.  The host solver returns the lowest state of the sector whatever its
spin.

``torch`` only allocates and views; per Davidson iteration O(space^2) scalars reach the host.
"""

from __future__ import annotations

import itertools
import time
from math import comb

import numpy as np

from .exceptions import NbedDriverError

DEVICE_BYTES = 288 * 10**9  # HBM of one MI355X: what memory_plan sizes the chunks for when nothing else is given
MAX_SPACE = 16              # nbx_lincomb / nbx_dots take up to 16 vectors
MAX_ROW = 13 * 1024         # beta strings in a row the kernels stage in LDS (csrc/fci.hip)
COMPUTE_UNITS = 256         # of one MI355X: what default_slabs fills


# ---------------------------------------------------------------- strings and link tables (host, a few MB)
def strings(n: int, k: int) -> np.ndarray:
    """Bit masks of the C(n, k) strings in rank order."""
    return np.array([sum(1 << p for p in occ) for occ in itertools.combinations(range(n), k)], dtype=np.int64)


def string_rank(n: int, occ) -> int:
    """Rank of the string with the ascending occupied orbitals ``occ`` (combinatorial number system)."""
    occ = sorted(int(p) for p in occ)
    k = len(occ)
    if len(set(occ)) != k or (occ and (occ[0] < 0 or occ[-1] >= n)):
        raise ValueError(f"string_rank: distinct orbitals in [0, {n}) expected")
    return comb(n, k) - 1 - sum(comb(n - 1 - p, k - i) for i, p in enumerate(occ))


def link_table(n: int, k: int) -> np.ndarray:
    """(C(n,k), n*n) int32: entry [S, p*n + q] is sign * (rank + 1) of E_pq |S> = a+_p a_q |S>, 0 where it vanishes.
    Every string has k (n - k + 1) non-zero entries."""
    masks = strings(n, k)
    order = np.argsort(masks)
    sorted_masks = masks[order]
    table = np.zeros((masks.size, n * n), dtype=np.int32)
    for p in range(n):
        for q in range(n):
            has_q = (masks >> q) & 1 == 1
            if p == q:
                table[has_q, p * n + q] = np.flatnonzero(has_q) + 1
                continue
            ok = has_q & ((masks >> p) & 1 == 0)
            src = masks[ok]
            new = (src ^ (1 << q)) | (1 << p)
            lo, hi = min(p, q), max(p, q)
            between = ((1 << hi) - 1) ^ ((1 << (lo + 1)) - 1)
            parity = np.array([bin(int(x)).count("1") & 1 for x in src & between], dtype=np.int64)
            target = order[np.searchsorted(sorted_masks, new)]
            table[ok, p * n + q] = (1 - 2 * parity) * (target + 1)
    return table


def interleave_signs(n: int, na: int, nb: int) -> np.ndarray:
    """(Na, Nb) of +-1: this module's determinant (alpha creators, then beta creators) over ``fci.ground_state``'s
    (creators in the order of the interleaved spin-orbital index 2p + s)."""
    sa, sb = strings(n, na), strings(n, nb)
    out = np.ones((sa.size, sb.size))
    for ia, ma in enumerate(sa):
        for ib, mb in enumerate(sb):
            # alpha p stands behind beta q in the interleaved order iff q < p
            swaps = sum(bin(int(mb) & ((1 << p) - 1)).count("1") for p in range(n) if (int(ma) >> p) & 1)
            if swaps & 1:
                out[ia, ib] = -1.0
    return out


# ---------------------------------------------------------------- memory plan
def memory_plan(n: int, na: int, nb: int, space: int = 12, chunk_rows: int | None = None, nroots: int = 1,
                capacity: int = DEVICE_BYTES) -> dict:
    """Bytes the device solver needs, by group, computed before anything is allocated (host arithmetic):

    vectors      the Davidson basis (``space`` vectors) and as many sigma vectors
    work         the diagonal, the residual, the correction and the 2 x nroots restart vectors
    tables       string masks and the two link tables (int32)
    hamiltonian  the spatial blocks and [G | k]
    chunk        D (2n^2 + 1, K) and E (2n^2, K) for the K = chunk_rows x Nb determinants of one chunk

    ``chunk_rows`` None: as many alpha rows as ``capacity`` (less a tenth) leaves room for, at least one and fewer
    than 2^31 determinants (one GEMM extent)."""
    n_a, n_b = comb(n, na), comb(n, nb)
    ndet = n_a * n_b
    g = 2 * n * n
    plan = {
        "vectors": 8 * 2 * space * ndet,
        "work": 8 * (3 + 2 * nroots) * ndet,
        "tables": 4 * (n_a * n * n + n * n * n_b + n_a + n_b),
        "hamiltonian": 8 * (3 * n**4 + 2 * n * n + g * (g + 1)),
    }
    per_row = 8 * (2 * g + 1) * n_b
    if chunk_rows is None:
        room = int(0.9 * capacity) - sum(plan.values())
        chunk_rows = max(1, min(n_a, room // per_row, (2**31 - 1) // n_b))
    chunk_rows = int(chunk_rows)
    if not 1 <= chunk_rows <= n_a:
        raise ValueError(f"chunk_rows must lie in [1, {n_a}]")
    plan["chunk"] = per_row * chunk_rows
    plan["total"] = sum(plan.values())
    plan["chunk_rows"] = chunk_rows
    plan["chunks"] = -(-n_a // chunk_rows)
    plan["ndet"] = ndet
    return plan


def default_slabs(n: int) -> int:
    """Partial matrices the D_b D_c^T of the densities is split into: the output is (2n^2 + 1)^2, a few 128 x 128 tiles
    at most, and the reduction runs over up to 2^31 determinants -- enough slabs that the batched GEMM launches at
    least one workgroup per compute unit whichever tile ``nbx_gemm`` picks (128 is its largest)."""
    tiles = (-(-(2 * n * n + 1) // 128)) ** 2
    return -(-COMPUTE_UNITS // tiles)


def memory_plan_rdm(n: int, na: int, nb: int, transition: bool = False, chunk_rows: int | None = None,
                    slabs: int | None = None, direct_only: bool = False, capacity: int = DEVICE_BYTES) -> dict:
    """Bytes the densities need, by group, computed before anything is allocated (host arithmetic):

    vectors        the ket, and the bra of a transition density
    tables         the two link tables (int32)
    direct         the (Na, 2n^2) partials of the 1-RDM kernel
    output         dm1, dm2 and the overlap
    slab_partials  ``slabs`` matrices (2n^2 + 1)^2 that the split reduction accumulates into   } not with
    d              D (2n^2 + 1, K) of one chunk of K = chunk_rows x Nb determinants, twice for a  } ``direct_only``
                   transition density

    ``chunk_rows`` None: as many alpha rows as ``capacity`` (less a tenth) leaves room for, at least one and fewer
    than 2^31 determinants (one GEMM extent).  ``slabs`` None: ``default_slabs(n)``."""
    n_a, n_b = comb(n, na), comb(n, nb)
    ndet = n_a * n_b
    g1 = 2 * n * n + 1
    nvec = 2 if transition else 1
    slabs = default_slabs(n) if slabs is None else int(slabs)
    if not 1 <= slabs <= 65535:
        raise ValueError("slabs must lie in [1, 65535]")
    plan = {
        "vectors": 8 * nvec * ndet,
        "tables": 4 * (n_a * n * n + n * n * n_b),
        "direct": 8 * n_a * (g1 - 1),
        "output": 8 * ((g1 - 1) + (0 if direct_only else 3 * n**4 + 1)),
        "slab_partials": 0 if direct_only else 8 * slabs * g1 * g1,
    }
    per_row = 8 * nvec * g1 * n_b
    if chunk_rows is None:
        room = int(0.9 * capacity) - sum(plan.values())
        chunk_rows = max(1, min(n_a, room // per_row, (2**31 - 1) // n_b))
    chunk_rows = int(chunk_rows)
    if not 1 <= chunk_rows <= n_a:
        raise ValueError(f"chunk_rows must lie in [1, {n_a}]")
    plan["d"] = 0 if direct_only else per_row * chunk_rows
    plan["total"] = sum(plan.values())
    plan["chunk_rows"] = chunk_rows
    plan["chunks"] = -(-n_a // chunk_rows)
    plan["slabs"] = slabs
    plan["ndet"] = ndet
    return plan


def _device_backend(backend):
    if backend is None:
        from .backend import get_backend

        backend = get_backend()
    if not hasattr(backend, "fci_gather"):
        raise NbedDriverError(f"the device FCI needs a HipBackend (got {type(backend).__name__})")
    return backend


def _unpack(spatial):
    if hasattr(spatial, "two_body"):
        return spatial.constant, spatial.one_body, spatial.two_body
    return spatial


def _diagonal(be, n, str_a, str_b, one, two, constant):
    return be.fci_diag(n, be.int_array(str_a), be.int_array(str_b), one, two, float(constant))


def _tables(be, n, na, nb):
    """String masks (host) and the link tables as the kernels read them (device): alpha (Na, n^2), beta transposed
    (n^2, Nb).  One construction for the sigma build and the densities."""
    return strings(n, na), strings(n, nb), be.int_array(link_table(n, na)), be.int_array(link_table(n, nb).T)


class SigmaBuilder:
    """H c for one Hamiltonian and one (n_alpha, n_beta) sector: tables, [G | k] and the chunk buffers, made once."""

    def __init__(self, be, spatial, nelec, space: int = 12, nroots: int = 1, chunk_rows: int | None = None):
        constant, one, two = _unpack(spatial)
        self.be = be
        self.constant = float(constant)
        self.n = n = int(one.shape[-1])
        self.na, self.nb = na, nb = int(nelec[0]), int(nelec[1])
        if not (1 <= n <= 31 and 0 <= na <= n and 0 <= nb <= n):
            raise ValueError(f"device FCI: 1 <= n <= 31 orbitals and 0 <= electrons per spin <= n expected (n = {n}, {nelec})")
        self.n_a, self.n_b = comb(n, na), comb(n, nb)
        self.ndet = self.n_a * self.n_b
        if self.n_b > MAX_ROW:
            raise NbedDriverError(f"device FCI: {self.n_b} beta strings per row exceed the {MAX_ROW} the kernels stage in LDS")
        held = 8 * 3 * n**4 if be.torch.is_tensor(two) and two.is_cuda else 0  # (device blocks are there already)
        free = be.free_bytes()
        self.plan = memory_plan(n, na, nb, space, chunk_rows, nroots, capacity=free + held)
        if self.plan["total"] - held > free:
            raise NbedDriverError(
                f"device FCI of {n} orbitals with ({na}, {nb}) electrons, {self.ndet} determinants, needs "
                f"{self.plan['total'] - held} bytes of device memory ({self.plan['vectors']} for {space} basis and sigma "
                f"vectors, {self.plan['work']} of work vectors, {self.plan['chunk']} for D and E of "
                f"{self.plan['chunk_rows']} alpha rows, {self.plan['tables']} of tables); {free} are free")
        self.rows = self.plan["chunk_rows"]
        self.one, self.two = be.asarray(one), be.asarray(two)
        self.str_a, self.str_b, self.link_a, self.link_bt = _tables(be, n, na, nb)
        self.g = be.fci_gmat(self.one, self.two)
        g = 2 * n * n
        self.d = be.empty((g + 1) * self.rows * self.n_b)
        self.e = be.empty(g * self.rows * self.n_b)
        self.seconds = None  # set to {"gather": 0.0, "gemm": 0.0, "scatter": 0.0} to time the phases (synchronises)

    def diagonal(self):
        """H_II on the device, (Na, Nb)."""
        return _diagonal(self.be, self.n, self.str_a, self.str_b, self.one, self.two, self.constant)

    def _timed(self, key, fn, *args):
        if self.seconds is None:
            return fn(*args)
        self.be.synchronize()
        t0 = time.perf_counter()
        fn(*args)
        self.be.synchronize()
        self.seconds[key] += time.perf_counter() - t0

    def __call__(self, c, out=None):
        """``out`` (Na, Nb) = H c; ``c`` is not modified and must not be ``out``."""
        be, n, g = self.be, self.n, 2 * self.n * self.n
        if c.numel() != self.ndet:
            raise ValueError(f"sigma: a vector of {self.ndet} determinants expected")
        if out is None:
            out = be.empty((self.n_a, self.n_b))
        for row0 in range(0, self.n_a, self.rows):
            rows = min(self.rows, self.n_a - row0)
            cols = rows * self.n_b
            d, e = self.d[: (g + 1) * cols], self.e[: g * cols]
            self._timed("gather", be.fci_gather, n, self.n_a, self.n_b, row0, rows, self.link_a, self.link_bt, c, d)
            self._timed("gemm", be.gemm_raw, "N", "N", g, cols, g + 1, 1.0, self.g, g + 1, 0, d, cols, 0, 0.0, e, cols, 0, 1)
            self._timed("scatter", be.fci_scatter, n, self.n_a, self.n_b, row0, rows, self.link_a, self.link_bt, e,
                        self.constant, c, row0 > 0, out)
        return out


def sigma(spatial, nelec, c, backend=None, chunk_rows: int | None = None):
    """H c on the device for a host or device vector ``c`` of shape (Na, Nb): the device array (Na, Nb)."""
    be = _device_backend(backend)
    sb = SigmaBuilder(be, spatial, nelec, space=1, chunk_rows=chunk_rows)
    return sb(be.asarray(c).reshape(sb.n_a, sb.n_b))


def diagonal(spatial, nelec, backend=None):
    """H_II on the device, (Na, Nb)."""
    be = _device_backend(backend)
    constant, one, two = _unpack(spatial)
    n = int(one.shape[-1])
    return _diagonal(be, n, strings(n, int(nelec[0])), strings(n, int(nelec[1])), be.asarray(one), be.asarray(two), constant)


# ---------------------------------------------------------------- densities
# Between a bra b and a ket c of one sector (a state density is b = c), in the blocks and index order of
# SpatialHamiltonian:  dm1[s][p,q] = <b| a+_ps a_qs |c>,  dm2[x][p,q,r,s] = <b| a+_ps a+_qt a_rt a_ss |c> for
# (s,t) = aa, bb, ab; the ba block is dm2[2][q,p,s,r].  With D_x = fci_gather(x) (x itself in the last row)
#     Graw = D_b D_c^T:  Graw[(s,kl),(t,mn)] = <b| E^s_lk E^t_mn |c>,  Graw[(s,kl), last] = <b| E^s_lk |c>,
# and a+_ps a+_qt a_rt a_ss = E^s_ps E^t_qr - delta_st delta_qs E^s_pr is the index map of nbx_fci_rdm_finish.
def _host(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


class RdmBuilder:
    """Densities of one (n_alpha, n_beta) sector: tables made once, buffers at the first use of each route.

    ``rdm12``: per chunk of alpha rows a gather of the ket (and of the bra, if it is another vector), then
    Graw += D_b D_c^T on the matrix cores, the reduction over the chunk's determinants cut into ``slabs`` contiguous
    ranges that each add into a partial matrix of their own (one batched ``nbx_gemm``, the ragged last range a second
    call); ``nbx_fci_rdm_finish`` adds the partials in a fixed order.  ``rdm1``: the direct kernel, no D.
    ``transition``: plan for two D buffers; ``direct_only``: plan for none.  ``held``: bytes of the plan's vectors that
    are on the device already."""

    def __init__(self, be, n, nelec, chunk_rows: int | None = None, slabs: int | None = None, transition: bool = False,
                 direct_only: bool = False, held: int = 0):
        self.be = be
        self.n = n = int(n)
        self.na, self.nb = na, nb = int(nelec[0]), int(nelec[1])
        if not (1 <= n <= 31 and 0 <= na <= n and 0 <= nb <= n):
            raise ValueError(f"device FCI: 1 <= n <= 31 orbitals and 0 <= electrons per spin <= n expected (n = {n}, {nelec})")
        self.n_a, self.n_b = comb(n, na), comb(n, nb)
        self.ndet = self.n_a * self.n_b
        if self.n_b > MAX_ROW:
            raise NbedDriverError(f"device FCI: {self.n_b} beta strings per row exceed the {MAX_ROW} the kernels stage in LDS")
        self.transition, self.direct_only = bool(transition), bool(direct_only)
        self.plan = self._fit(self.transition, self.direct_only, chunk_rows, slabs, int(held))
        self.rows, self.slabs = self.plan["chunk_rows"], self.plan["slabs"]
        self.str_a, self.str_b, self.link_a, self.link_bt = _tables(be, n, na, nb)
        self.d = [None, None]
        self.graw = self.partial = None
        self.seconds = None  # set to {"gather": 0.0, "gemm": 0.0, "finish": 0.0} to time the phases (synchronises)

    def _fit(self, transition, direct_only, chunk_rows, slabs, held):
        free = self.be.free_bytes()
        plan = memory_plan_rdm(self.n, self.na, self.nb, transition, chunk_rows, slabs, direct_only, capacity=free + held)
        if plan["total"] - held > free:
            raise NbedDriverError(
                f"densities of {self.n} orbitals with ({self.na}, {self.nb}) electrons, {self.ndet} determinants, need "
                f"{plan['total'] - held} bytes of device memory ({plan['vectors']} of vectors, {plan['d']} for "
                f"{2 if transition else 1} D of {plan['chunk_rows']} alpha rows, {plan['slab_partials']} for "
                f"{plan['slabs']} slab partials, {plan['direct']} of 1-RDM partials, {plan['tables']} of tables, "
                f"{plan['output']} of output); {free} are free")
        return plan

    def _vector(self, v, what):
        shape = tuple(v.shape) if hasattr(v, "shape") else np.shape(v)
        if shape != (self.n_a, self.n_b) and shape != (self.ndet,):
            raise ValueError(f"{what}: a vector of shape ({self.n_a}, {self.n_b}) expected, got {shape}")
        return self.be.asarray(v).reshape(self.n_a, self.n_b)

    def _pair(self, c, bra):
        """(bra, ket) on the device; the bra IS the ket where none is given."""
        ket = self._vector(c, "ket")
        return (ket if bra is None or bra is c else self._vector(bra, "bra")), ket

    def _timed(self, key, fn, *args):
        if self.seconds is None:
            return fn(*args)
        self.be.synchronize()
        t0 = time.perf_counter()
        out = fn(*args)
        self.be.synchronize()
        self.seconds[key] += time.perf_counter() - t0
        return out

    def rdm1(self, c, bra=None):
        """dm1 (2, n, n) on the device by the direct kernel."""
        be = self.be
        b, k = self._pair(c, bra)
        if self.partial is None:
            self.partial = be.empty((self.n_a, 2 * self.n * self.n))
        return be.fci_rdm1(self.n, self.n_a, self.n_b, self.link_a, self.link_bt, b, k, self.partial)

    def rdm12(self, c, bra=None):
        """(dm1 (2,n,n), dm2 (3,n,n,n,n), overlap (1,)) on the device."""
        be, n, g1 = self.be, self.n, 2 * self.n * self.n + 1
        if self.direct_only:
            raise NbedDriverError("this RdmBuilder was planned for the 1-RDM alone (direct_only)")
        b, k = self._pair(c, bra)
        two = b is not k
        if two and not self.transition:  # a second D after all: the same chunks must still fit
            there = (self.d[0], self.graw, self.partial)
            held = 16 * self.ndet + self.plan["tables"] + sum(8 * t.numel() for t in there if t is not None)
            self._fit(True, False, self.rows, self.slabs, held)
            self.transition = True
        if self.graw is None:
            self.graw = be.zeros((self.slabs, g1, g1))
        else:
            self.graw.zero_()
        for i in range(2 if two else 1):
            if self.d[i] is None:
                self.d[i] = be.empty(g1 * self.rows * self.n_b)
        for row0 in range(0, self.n_a, self.rows):
            rows = min(self.rows, self.n_a - row0)
            cols = rows * self.n_b
            dk = self.d[0][: g1 * cols]
            self._timed("gather", be.fci_gather, n, self.n_a, self.n_b, row0, rows, self.link_a, self.link_bt, k, dk)
            db = dk
            if two:
                db = self.d[1][: g1 * cols]
                self._timed("gather", be.fci_gather, n, self.n_a, self.n_b, row0, rows, self.link_a, self.link_bt, b, db)
            self._timed("gemm", self._accumulate, db, dk, cols)
        return self._timed("finish", be.fci_rdm_finish, n, self.slabs, self.graw)

    def _accumulate(self, db, dk, cols):
        """graw[z] += D_b[:, slab z] D_c[:, slab z]^T.  Every partial starts from zero and is only ever added to, by
        the chunks in ascending order: a fixed order of additions per element."""
        be, g1 = self.be, 2 * self.n * self.n + 1
        ks = -(-cols // self.slabs)
        full = cols // ks
        rem = cols - full * ks
        be.gemm_raw("N", "T", g1, g1, ks, 1.0, db, cols, ks, dk, cols, ks, 1.0, self.graw, g1, g1 * g1, full)
        if rem:
            be.gemm_raw("N", "T", g1, g1, rem, 1.0, db[full * ks:], cols, 0, dk[full * ks:], cols, 0, 1.0, self.graw[full],
                        g1, 0, 1)


def _held(be, *vectors):
    return sum(8 * v.numel() for v in vectors if v is not None and be.torch.is_tensor(v) and v.is_cuda)


def rdm1(c, n, nelec, bra=None, backend=None):
    """dm1 (2, n, n) = <bra| a+_ps a_qs |c> on the device by the direct kernel (no D buffer); ``c`` and ``bra`` are
    host or device vectors (Na, Nb) in this module's determinant convention, ``bra`` None a state density."""
    be = _device_backend(backend)
    rb = RdmBuilder(be, n, nelec, transition=bra is not None and bra is not c, direct_only=True, held=_held(be, c, bra))
    return rb.rdm1(c, bra)


def rdm12(c, n, nelec, bra=None, backend=None, chunk_rows: int | None = None, slabs: int | None = None):
    """(dm1 (2,n,n), dm2 (3,n,n,n,n)) on the device by gather, GEMM and finish."""
    be = _device_backend(backend)
    rb = RdmBuilder(be, n, nelec, chunk_rows, slabs, transition=bra is not None and bra is not c, held=_held(be, c, bra))
    dm1, dm2, _ = rb.rdm12(c, bra)
    return dm1, dm2


def spin_square(dm2, nelec) -> float:
    """<S^2> = S_z (S_z + 1) + n_beta - sum_pq dm2[ab][p,q,p,q] of a normalised state, S_z = (n_alpha - n_beta) / 2."""
    na, nb = int(nelec[0]), int(nelec[1])
    ab = _host(dm2[2])
    sz = 0.5 * (na - nb)
    return float(sz * (sz + 1.0) + nb - np.einsum("pqpq->", ab))


def energy_from_rdm(spatial, dm1, dm2, overlap: float = 1.0) -> float:
    """<b|H|c> = constant <b|c> + sum one_body dm1 + sum two_body[aa] dm2[aa] + sum two_body[bb] dm2[bb]
    + 2 sum two_body[ab] dm2[ab] (host arithmetic on host copies)."""
    constant, one, two = _unpack(spatial)
    one, two, dm1, dm2 = _host(one), _host(two), _host(dm1), _host(dm2)
    return float(float(constant) * float(overlap) + np.sum(one * dm1) + np.sum(two[0] * dm2[0]) + np.sum(two[1] * dm2[1])
                 + 2.0 * np.sum(two[2] * dm2[2]))


class FCIGpuResult:
    """Duck-types ``fci.FCIResult``: ``e_tot``, ``energies``, ``converged``, ``determinants``; ``ci`` (Na, Nb) -- for
    nroots > 1 (nroots, Na, Nb) -- is copied to the host on first access.  The density methods (``rdm1``, ``rdm12``,
    ``trans_rdm1``, ``trans_rdm12``, ``spin_square``, ``natural_occupations``) return host arrays in the conventions
    of ``rdm12`` above."""

    def __init__(self, be, energies, ci_dev, converged, iterations, residual_norm, strings_a, strings_b, n):
        self._be, self._ci_dev, self._ci, self._rdm = be, ci_dev, None, None
        self.energies = np.asarray(energies, dtype=float)
        self.e_tot = float(self.energies[0])
        self.converged = bool(converged)
        self.iterations = int(iterations)
        self.residual_norm = residual_norm
        self.strings_a, self.strings_b = strings_a, strings_b
        self.norb = n

    @property
    def ci(self):
        if self._ci is None:
            self._ci = np.array(self._be.to_host(self._ci_dev))
            self._ci_dev = None
        return self._ci

    @property
    def determinants(self):
        """Interleaved spin-orbital masks (alpha on the even bits) in the order of ``ci.ravel()``."""
        def spread(m):
            return sum(((int(m) >> p) & 1) << (2 * p) for p in range(self.norb))

        return [spread(a) | (spread(b) << 1) for a in self.strings_a for b in self.strings_b]

    # -- densities: the device copy of the vector while it exists, the host copy uploaded again once ``ci`` has dropped it
    @property
    def nelec(self):
        return bin(int(self.strings_a[0])).count("1"), bin(int(self.strings_b[0])).count("1")

    def _roots(self, i, j):
        """Roots i and j as device vectors (Na, Nb); both are checked before anything is uploaded."""
        nroots = int(self.energies.size)
        for root in (i, j):
            if not (isinstance(root, (int, np.integer)) and 0 <= root < nroots):
                raise ValueError(f"root {root!r}: this result holds {nroots} root(s)")
        v = self._ci_dev if self._ci_dev is not None else self._be.asarray(self._ci)
        v = v.reshape(nroots, len(self.strings_a), len(self.strings_b))
        return v[int(i)], v[int(j)]

    def _builder(self):
        if self._rdm is None:
            held = 8 * len(self.strings_a) * len(self.strings_b) if self._ci_dev is not None else 0
            self._rdm = RdmBuilder(self._be, self.norb, self.nelec, held=held)
        return self._rdm

    def trans_rdm12(self, i, j):
        """(dm1, dm2) with dm1[s][p,q] = <i| a+_ps a_qs |j> between roots i and j, host arrays."""
        bra, ket = self._roots(i, j)
        dm1, dm2, _ = self._builder().rdm12(ket, None if i == j else bra)
        return self._be.to_host(dm1), self._be.to_host(dm2)

    def trans_rdm1(self, i, j):
        bra, ket = self._roots(i, j)
        return self._be.to_host(self._builder().rdm1(ket, None if i == j else bra))

    def rdm1(self, root=0):
        """dm1 (2, n, n) of a root by the direct kernel (no D buffer), a host array."""
        return self.trans_rdm1(root, root)

    def rdm12(self, root=0):
        """(dm1 (2,n,n), dm2 (3,n,n,n,n)) of a root, host arrays."""
        return self.trans_rdm12(root, root)

    def spin_square(self, root=0) -> float:
        return spin_square(self.rdm12(root)[1], self.nelec)

    def natural_occupations(self, root=0) -> np.ndarray:
        """Eigenvalues of dm1[alpha] + dm1[beta], descending."""
        dm1 = self.rdm1(root)
        total = dm1[0] + dm1[1]
        return np.linalg.eigvalsh(0.5 * (total + total.T))[::-1].copy()


def solve(constant, h1, h2, nelec, **kwargs) -> FCIGpuResult:
    """``solve_spatial`` from the dense spin-orbital tensors of ``build()`` (direct use and tests; the driver calls
    ``solve_spatial``, which never holds a (2n)^4 tensor)."""
    from .ccsd_gpu import spatial_from_dense

    one, two = spatial_from_dense(h1, h2)
    return solve_spatial((constant, one, two), nelec, **kwargs)


def solve_spatial(spatial, nelec, occupied=None, conv_tol: float = 1e-10, max_cycle: int = 200, space: int = 12,
                  nroots: int = 1, backend=None, chunk_rows: int | None = None, stats: dict | None = None) -> FCIGpuResult:
    """Lowest ``nroots`` states of the (n_alpha, n_beta) = ``nelec`` sector by restarted subspace Davidson with the
    diagonal preconditioner, converged on the residual 2-norm.

    ``spatial``: a ``SpatialHamiltonian`` or ``(constant, one_body, two_body)`` as host or device arrays.  ``occupied``:
    the spin orbitals (index 2p + s, alpha even) of the start determinant; None starts from the lowest diagonal
    element.  ``space``: most basis vectors kept before the basis is collapsed onto the current Ritz vectors.  See the
    module docstring on the spin symmetry of the start vector.  ``stats``, if given, receives the memory plan, the
    residual history and the seconds per iteration."""
    be = _device_backend(backend)
    nroots = int(nroots)
    if not (1 <= nroots < space <= MAX_SPACE):
        raise ValueError(f"1 <= nroots < space <= {MAX_SPACE} expected")
    sb = SigmaBuilder(be, spatial, nelec, space=space, nroots=nroots, chunk_rows=chunk_rows)
    n, na, nb, ndet = sb.n, sb.na, sb.nb, sb.ndet
    if nroots > ndet:
        raise ValueError(f"{nroots} roots asked of {ndet} determinants")
    if stats is not None:
        stats.update(plan=sb.plan, ndet=ndet)
    diag = sb.diagonal()
    flat_diag = diag.view(-1)
    start = []
    if occupied is not None:
        occ = sorted(int(i) for i in occupied)
        occ_a, occ_b = [i >> 1 for i in occ if i % 2 == 0], [i >> 1 for i in occ if i % 2 == 1]
        if len(occ_a) != na or len(occ_b) != nb:
            raise ValueError(f"occupied holds {len(occ_a)} + {len(occ_b)} spin orbitals, nelec is {(na, nb)}")
        start.append(string_rank(n, occ_a) * sb.n_b + string_rank(n, occ_b))
    if len(start) < nroots or not start:
        lowest = be.torch.topk(flat_diag, min(ndet, nroots + 1), largest=False).indices.tolist()
        start += [i for i in lowest if i not in start][: nroots - len(start)]
    if ndet == 1:
        e0 = float(be.read_scalars(flat_diag)[0])
        return FCIGpuResult(be, [e0], be.asarray(np.ones((1, 1))), True, 0, 0.0, sb.str_a, sb.str_b, n)

    space = min(space, ndet)
    basis, sig = be.empty((space, ndet)), be.empty((space, ndet))
    res, cor = be.empty(ndet), be.empty(ndet)
    keep = be.empty((2, nroots, ndet))
    hsub = np.zeros((space, space))

    def append(m):
        """sigma of basis vector m and its row / column of the subspace matrix."""
        sb(basis[m], sig[m].view(sb.n_a, sb.n_b))
        col = be.dots(sig[m], basis[: m + 1])
        hsub[: m + 1, m] = col
        hsub[m, : m + 1] = col

    m = 0
    for idx in start:
        basis[m].zero_()
        basis[m, idx] = 1.0
        append(m)
        m += 1
    def residual(theta_k, y_k):
        """``res`` = (H - theta) x for the Ritz vector x = sum y_k[i] basis[i]; returns its 2-norm."""
        be.lincomb(y_k, sig[: len(y_k)], out=res)
        be.lincomb(y_k, basis[: len(y_k)], out=cor)
        be.axpby(-float(theta_k), cor, 1.0, res)
        return float(np.sqrt(max(be.dots(res, res.view(1, -1))[0], 0.0)))

    converged, it, norms = False, 0, [float("inf")] * nroots
    history, seconds = [], []
    for it in range(1, max_cycle + 1):
        t_start = time.perf_counter()
        theta, y = np.linalg.eigh(hsub[:m, :m])
        target = None
        for k in range(nroots):
            norms[k] = residual(theta[k], y[:, k])
            if not norms[k] < conv_tol:  # (a NaN is "not converged")
                target = k
                break
        history.append(list(norms))
        if target is None:
            converged = True
            break
        if m == space:  # collapse the basis onto the Ritz vectors of the wanted roots
            for k in range(nroots):
                be.lincomb(y[:, k], basis[:m], out=keep[0, k])
                be.lincomb(y[:, k], sig[:m], out=keep[1, k])
            basis[:nroots].copy_(keep[0])
            sig[:nroots].copy_(keep[1])
            hsub[:] = 0.0
            hsub[np.arange(nroots), np.arange(nroots)] = theta[:nroots]
            m = nroots
            if m == space:  # (only where the sector has no more determinants than roots are asked for)
                break
        be.fci_precond(res, flat_diag, float(theta[target]), 1e-8, cor)
        for _ in range(2):  # classical Gram-Schmidt, twice
            overlap = be.dots(cor, basis[:m])
            be.lincomb(overlap, basis[:m], out=res)
            be.axpby(-1.0, res, 1.0, cor)
        norm = float(np.sqrt(max(be.dots(cor, cor.view(1, -1))[0], 0.0)))
        if not norm > 1e-14:  # nothing left outside the basis
            break
        be.lincomb([1.0 / norm], cor.view(1, -1), out=basis[m])
        append(m)
        m += 1
        seconds.append(time.perf_counter() - t_start)
    if not converged:  # the basis has changed since the last eigh (a vector appended, or collapsed): the Ritz pairs of what it is now
        theta, y = np.linalg.eigh(hsub[:m, :m])
        norms = [residual(theta[k], y[:, k]) for k in range(nroots)]
    if nroots == 1:
        ci = be.lincomb(y[:, 0], basis[:m], out=cor).view(sb.n_a, sb.n_b)
    else:
        for k in range(nroots):
            be.lincomb(y[:, k], basis[:m], out=keep[0, k])
        ci = keep[0].view(nroots, sb.n_a, sb.n_b)
    if stats is not None:
        stats.update(iterations=it, residual_history=history, iteration_seconds=seconds)
    return FCIGpuResult(be, theta[:nroots], ci, converged, it, norms[0] if nroots == 1 else list(norms), sb.str_a, sb.str_b,
                        n)
