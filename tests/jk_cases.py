"""Shared by tests/test_host_jk_cases.py (CPU), tests/test_gpu_jk_exact.py and tests/_jk_exact_worker.py (MI355X): a
two-electron tensor in factorised form whose J/K contraction and AO->MO transform float64 holds EXACTLY, host references
of O(L N^3) cost for every element at every size, and a size for every kernel instance behind nbx_jk_packed,
nbx_jk_dense, nbx_jk_dense_sym and the nbx_ao2mo* entry points.

The tensor.  (pq|rs) = sum_L B_L[p,q] B_L[r,s] with L = 3 symmetric integer factors: B_0 has entries in {+-1, +-3},
B_1 and B_2 in {-2, 0, 2}.  It has the 8-fold symmetry of real two-electron integrals, every entry is odd (odd x odd
plus two even terms) and therefore never zero -- a kernel cannot skip, screen or drop an integral without changing an
integer -- and an index order outside the 8-fold group, e.g. (pr|qs), agrees with (pq|rs) on a sixth of the entries only
(tests/test_host_jk_cases.py keeps that at or below a quarter).  The two densities are symmetric with odd entries from
two DIFFERENT ranges, {+-1, +-3} and {+-1, +-3, +-5}: exchanging the spins changes K.  hv has entries in [-4, 4].

Why every kernel has to return the reference in every bit.  Every term of every output element is an integer; the
weights the kernels apply are 2 (D_ab + D_ba for a != b), 1/2 (jk_m8.hip stores the element (rs) = (pq) of a tile
halved) and the sum K = Kp + Kp^T -- all dyadic, so every term stays an integer multiple of 1/2.  The sum of |terms| of
one element is at most

    J_pq :  sum_L |B_L[p,q]| sum_rs |B_L[r,s]| (|D^a_rs| + |D^b_rs|)        (9.1e6 at N = 400)
    K_pr :  sum_L (|B_L| |D^x| |B_L|)[p,r]                                    (4.1e6 at N = 400)

far below 2^52 (headroom() computes both; the host test asserts it for every case of the tables).  Every partial sum a
kernel can form, in any order, fused or not, split over lanes, waves, workgroups and slabs in any way, is then a float64:
no rounding ever happens, and numpy's float64 evaluation of the factorised formulas

    J    = sum_L B_L tr(B_L Dtot)             K[x] = sum_L B_L D[x] B_L
    (ij|kl) = sum_L (C1^T B_L C2)[i,j] (C3^T B_L C4)[k,l]

IS the answer.  The comparisons are assert_array_equal / torch.equal: a missing, doubled or misplaced integral, a
weight on the wrong diagonal class, swapped spins -- each changes an integer (tests/test_host_jk_cases.py runs these
mutations through a numpy restatement of the tile walk and checks that the comparison fails for each).

Graded variant.  Integer exponents e_p in [-12, 12]; B_L[p,q] is scaled by 2^(e_p + e_q) (the tensor by
2^(e_p + e_q + e_r + e_s)), D_qr by 2^-(e_q + e_r), hv_pq by 2^(e_p + e_q).  Every term of J_pq then carries the factor
2^(e_p + e_q) and every term of K_pr the factor 2^(e_p + e_r): the terms of ONE output element share one exponent,
their integer parts are those of the plain variant, and everything above still holds -- while the inputs span 2^96.
A kernel that orders, screens or truncates by magnitude fails it; so does one that adds terms of different elements.

Slab conventions (slab_reference).  A row slab [p0, p1) of
  * nbx_jk_dense                  : rows p0 .. p1-1 of J and K ("rows");
  * nbx_jk_dense_sym, jk_s4 / jk_m4 / jk_mx .hip : the pairs (p, q <= p), p in the slab, and their mirror images -- (ab|cd)
                                    with max(a, b) in the slab ("sym") -- with the K partial rows summed on and below
                                    the diagonal only and mirrored (jk_sym_reduce_kernel, k_lower):
                                    K_slab = tril(K_sym) + tril(K_sym, -1)^T ("lower"); an odd N of nbx_jk_dense_sym is
                                    nbx_jk_dense's rows scattered into full-size matrices;
  * jk_m8.hip (8-fold tiles)      : of tile (p, q) only (rs) <= (pq) is stored, every integral once with the weight of
                                    its whole orbit: (ab|cd) with max(a, b, c, d) in the slab ("fold8").  That tensor is
                                    the factorised one of B[:, :p1, :p1] minus that of B[:, :p0, :p0].
Each is additive over slabs and each is O(L N^3) on the host.

The case tables name, per entry, the kernel file and the instance the size is there for; the library's own routing
query (nbx_jk_packed_route) has to agree before a result is compared, and tests/test_host_jk_cases.py fails when an
instance the dispatch code can select has no entry.

Section "not exact" (a kernel that is inexact for a correct, documented reason is held to a derived bound instead):
empty -- no kernel needed it.
"""

from __future__ import annotations

import ctypes
from collections import namedtuple
from functools import lru_cache

import numpy as np

NONE, S4, M4, M8, MX, MX_HI = range(6)  # NBX_JK_KERNEL_* of include/nbx.h
KERNEL_NAMES = {NONE: "NONE", S4: "S4", M4: "M4", M8: "M8", MX: "MX", MX_HI: "MX_HI"}
NFACT = 3
EXP_RANGE = 12

# ------------------------------------------------------------------------------------------ packed J/K
# n: the size; kernel / run_as: what nbx_jk_packed_route has to answer; why: the instance the size is there for
Packed = namedtuple("Packed", "n kernel run_as why")

# jk_s4.hip (N <= 96): one size per (NB, loads per thread) instance -- s4_nb() gives NB = 4 when N % 4 == 0 and the
# chunks of N / 4 rows fill a staging slot, s4_lpt_class() the template's LPT in {2, 6, 10} (17 starts above 96, where
# jk_m8.hip has taken over: tests/_jk_exact_worker.py reaches it behind NBX_JK_M8=0 NBX_JK_M4=0) -- and a zero-padded
# size of each.  NB^2 LPT is what nbx_jk_dts_bytes() / 1024 says, which is how the host test knows the instance.
S4_CASES = [
    Packed(24, S4, 24, "NB=2 LPT=2, the smallest size the kernel has"),
    Packed(16, S4, 24, "NB=2 LPT=2 zero-padded by eight, the most s4_padded allows"),
    Packed(23, S4, 24, "NB=2 LPT=2 zero-padded (odd)"),
    Packed(26, S4, 26, "NB=2 LPT=2, N % 4 == 2, blocks of 13 rows"),
    Packed(32, S4, 32, "NB=4 LPT=2, the first"), Packed(31, S4, 32, "NB=4 LPT=2 zero-padded (odd)"),
    Packed(88, S4, 88, "NB=4 LPT=2, the last"),
    Packed(46, S4, 46, "NB=2 LPT=6, the first"), Packed(45, S4, 46, "NB=2 LPT=6 zero-padded (odd)"),
    Packed(78, S4, 78, "NB=2 LPT=10, the first"), Packed(77, S4, 78, "NB=2 LPT=10 zero-padded (odd)"),
    Packed(92, S4, 92, "NB=4 LPT=6, the first"), Packed(91, S4, 92, "NB=4 LPT=6 zero-padded (odd)"),
    Packed(96, S4, 96, "NB=4 LPT=6, the last size below jk_m8.hip"),
]
# NB^2 LPT of the instance each unpadded size above runs on (asserted by the host test against nbx_jk_dts_bytes / 1024)
S4_CLASSES = {24: 8, 26: 8, 32: 32, 88: 32, 46: 24, 78: 40, 92: 96, 96: 96}

# jk_m8.hip: NBX_M8_SIZES, N = 4 NB for NB = 25 .. 37, and three padded sizes with N mod 4 = 1, 2, 3
M8_INSTANCES = list(range(100, 149, 4))
M8_CASES = [Packed(n, M8, n, f"instance NB={n // 4}") for n in M8_INSTANCES] + [
    Packed(97, M8, 100, "N % 4 == 1 -> 100, the first size of the kernel"),
    Packed(126, M8, 128, "N % 4 == 2 -> 128"),
    Packed(147, M8, 148, "N % 4 == 3 -> 148, the bench's instance"),
]

# jk_mx.hip (NBX_MX_SIZES: NB = 38 .. 64 in steps of two) and jk_mx_hi.hip (NB = 68 .. 100 in steps of four): whole block
# rows per chunk up to N = 288 (MX_SPLIT_NB = 72), band segments from N = 304
MX_LO_INSTANCES = list(range(152, 257, 8))
MX_HI_INSTANCES = [272, 288] + list(range(304, 401, 16))
MX_CASES = ([Packed(n, MX, n, f"instance NB={n // 4}, whole block rows") for n in MX_LO_INSTANCES]
            + [Packed(n, MX_HI, n, f"instance NB={n // 4}, " + ("whole block rows" if n <= 288 else "band segments"))
               for n in MX_HI_INSTANCES]
            + [Packed(149, MX, 152, "the first size past jk_m8.hip, padded by three"),
               Packed(185, MX, 192, "whole-row instance, padded by seven (odd)"),
               Packed(190, MX, 192, "the same instance, padded by two"),
               Packed(264, MX_HI, 272, "padded by eight, the most nbx_jk_mx_padded allows"),
               Packed(297, MX_HI, 304, "band-segment instance, padded by seven (odd)"),
               Packed(302, MX_HI, 304, "the same instance, padded by two"),
               Packed(393, MX_HI, 400, "the furthest padding onto the largest instance")])

PACKED_CASES = S4_CASES + M8_CASES + MX_CASES
# from here on the dense tensor is built a slab at a time (dense + packed of N = 400 would need 256 GB)
SLAB_ONLY_FROM = 320
DENSE_SLAB_BYTES = 32 * 2 ** 30

# one instance per kernel family for the graded variant and the stale-LDS run
FAMILY_CASES = {"s4": 92, "m8": 116, "mx-whole": 168, "mx-hi-whole": 272, "mx-hi-band": 304}

# What the fallbacks behind the environment switches are handed (tests/_jk_exact_worker.py; the switches are read once
# per process).  NBX_JK_M8=0 NBX_JK_M4=0: nbx_jk_mx_padded looks eight rows ahead, so 144 .. 148 run zero-padded on
# jk_mx.hip's N = 152 instance and jk_s4.hip keeps 97 .. 143.
SWITCH_CASES = {
    "NBX_JK_M8=0": [Packed(n, M4, n, f"jk_m4.hip instance NB={n // 4}") for n in M8_INSTANCES]
                   + [Packed(97, M4, 100, "padded"), Packed(126, M4, 128, "padded"), Packed(147, M4, 148, "padded")],
    "NBX_JK_M8=0 NBX_JK_M4=0": [Packed(n, S4, n, "jk_s4.hip (NB=4, LPT 6 / 10 / 17)")
                                for n in range(100, 144, 4)]
                               + [Packed(144, MX, 152, "within eight of jk_mx.hip's first instance"),
                                  Packed(148, MX, 152, "within eight of jk_mx.hip's first instance"),
                                  Packed(97, S4, 98, "padded by one onto N = 98: NB=2, blocks of 49 rows"), Packed(126, S4, 128, "padded"),
                                  Packed(139, S4, 140, "padded")],
    "NBX_JK_MX=0": [Packed(n, S4, n, "jk_s4.hip (NB=4 LPT=17)") for n in MX_LO_INSTANCES]
                   + [Packed(149, S4, 152, "padded"), Packed(185, S4, 188, "padded onto a size jk_mx.hip has no instance for"),
                      Packed(190, S4, 192, "padded")],
}

# ------------------------------------------------------------------------------------------ dense J/K
# jk.hip: jk_plan() picks VEC2 = (N even), CS = 1 / 2 / 4 column segments for CX = N / 2 (even) or N (odd) columns per
# thread row up to 256 / 512 / beyond; jk_impl() has an instance per (NDM, CS, VEC2).  The smallest N of each class; the
# sizes past 256 run as row slabs only (the dense tensor of N = 514 is 558 GB).  rows: the slab the GPU test builds.
Dense = namedtuple("Dense", "n cs vec2 rows why")
DENSE_CASES = [
    Dense(2, 1, True, None, "CS=1 VEC2, the smallest even size"),
    Dense(48, 1, True, None, "CS=1 VEC2, several row groups per workgroup"),
    Dense(1, 1, False, None, "CS=1 scalar columns, the smallest odd size"),
    Dense(37, 1, False, None, "CS=1 scalar columns, an odd size"),
    Dense(257, 2, False, (100, 103), "CS=2 scalar columns, the smallest"),
    Dense(513, 4, False, (255, 257), "CS=4 scalar columns, the smallest"),
    Dense(514, 2, True, (300, 302), "CS=2 VEC2, the smallest"),
    Dense(1026, 4, True, (1000, 1001), "CS=4 VEC2, the smallest"),
]

# jk_sym.hip: js_qb() = 2 up to N = 192 and 4 beyond; even N with N / 2 <= 256 threads; odd N falls back to nbx_jk_dense
Sym = namedtuple("Sym", "n qb rows why")
SYM_CASES = [
    Sym(24, 2, None, "QB=2, whole tensor"),
    Sym(192, 2, None, "QB=2, the last size"),
    Sym(194, 4, None, "QB=4, the first size"),
    Sym(512, 4, (509, 512), "QB=4, the largest N / 2 the kernel has threads for; the last rows (the longest tile rows)"),
    Sym(37, 0, None, "odd: the fallback through nbx_jk_dense and the row scatter"),
]


def dense_class(n: int):
    """(CS, VEC2) of jk_plan (csrc/jk.hip) for this size."""
    vec2 = n % 2 == 0
    cx = n // 2 if vec2 else n
    return (1 if cx <= 256 else 2 if cx <= 512 else 4), vec2


def sym_qb(n: int) -> int:
    """QB of js_qb (csrc/jk_sym.hip); 0: no symmetric kernel (odd N, or more than 256 column pairs)."""
    if n < 2 or n % 2 or n // 2 > 256:
        return 0
    return 2 if n <= 192 else 4


# ------------------------------------------------------------------------------------------ ao2mo
# (N; n1, n2, n3, n4): the four quarters are GEMMs of 32 / 64 / 128 tiles (tests/gemm_cases.py), so the extents cross a
# tile edge of each size, are odd, unequal, below and above the 64-column instance, exactly 128 and 128 + 2
Ao2mo = namedtuple("Ao2mo", "n n1 n2 n3 n4 why")
AO2MO_CASES = [
    Ao2mo(24, 9, 9, 8, 8, "small, one tile"),
    Ao2mo(37, 7, 7, 5, 11, "odd N, unequal odd extents"),
    Ao2mo(80, 72, 72, 72, 72, "the > 64-column instance"),
    Ao2mo(148, 128, 128, 128, 128, "the bench shape"),
    Ao2mo(148, 130, 130, 130, 130, "one full 128 tile and a partial one"),
]


# ------------------------------------------------------------------------------------------ routing
def route(lib, n: int):
    """(kernel, run_as) of nbx_jk_packed_route."""
    k, r = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = lib.nbx_jk_packed_route(n, ctypes.byref(k), ctypes.byref(r))
    assert rc == 0, rc
    return k.value, r.value


def packed_id(c) -> str:
    return f"{KERNEL_NAMES[c.kernel]}-{c.n}" + (f"as{c.run_as}" if c.run_as != c.n else "")


# ------------------------------------------------------------------------------------------ the size queries
# tests/golden/jk_packed_sizes.json (tests/golden/make_jk_packed_sizes.py, tests/test_host_jk_packed_sizes.py): what the
# host-arithmetic queries of the packed J/K answer for every size, under the default and under these switch settings
# (the last one is where jk_mx.hip takes 144 .. 148 although jk_m8.hip covers them)
SIZE_SETTINGS = ["", *SWITCH_CASES, "NBX_JK_M4=0"]
SIZE_RANGE = 421


def size_slabs(n: int):
    """The row ranges the byte counts are asked for: the whole tensor, then the slabs of equal_work_cuts."""
    return [(0, n)] + equal_work_cuts(n)


def packed_size_answers(lib) -> dict:
    """Per query, one entry per n in range(SIZE_RANGE); packed_bytes / worksize: one number per slab of size_slabs(n)
    (worksize: for ndm = 1, then for ndm = 2)."""
    sizes = range(SIZE_RANGE)
    routes = [route(lib, n) for n in sizes]
    return {
        "supported": [lib.nbx_jk_packed_supported(n) for n in sizes],
        "fold": [lib.nbx_jk_packed_fold(n) for n in sizes],
        "kernel": [k for k, _ in routes],
        "run_as": [r for _, r in routes],
        "dts_bytes": [lib.nbx_jk_dts_bytes(n) for n in sizes],
        "packed_bytes": [[lib.nbx_eri_packed_bytes(n, p0, p1) for p0, p1 in size_slabs(n)] for n in sizes],
        "worksize": [[lib.nbx_jk_packed_worksize(n, p0, p1, ndm) for ndm in (1, 2) for p0, p1 in size_slabs(n)]
                     for n in sizes],
    }


def packed_size_answers_in_child(setting: str) -> dict:
    """packed_size_answers of the built library in a fresh process under `setting` (the switches are read once per
    process; host arithmetic only, no GPU)."""
    import json
    import os
    import subprocess
    import sys

    code = ("import json, sys; sys.path.insert(0, sys.argv[1]); import jk_cases as jc; from nbed_amd import _nbx; "
            "print('SIZES', json.dumps(jc.packed_size_answers(_nbx.load_library())))")
    tests = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, PYTHONPATH=os.path.dirname(tests))
    for name in ("NBX_JK_M8", "NBX_JK_M4", "NBX_JK_MX"):
        env.pop(name, None)
    env.update(item.split("=") for item in setting.split())
    r = subprocess.run([sys.executable, "-c", code, tests], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads(r.stdout.rsplit("SIZES", 1)[1])


# ------------------------------------------------------------------------------------------ operands
Operands =namedtuple("Operands", "b dm hv e")


def _sym_choice(rng, values, n):
    a = rng.choice(np.asarray(values, dtype=np.float64), size=(n, n))
    return np.tril(a) + np.tril(a, -1).T


@lru_cache(maxsize=4)
def operands(n: int, seed: int = 0) -> Operands:
    """B (3, N, N), D (2, N, N), hv (2, N, N), all symmetric and integer valued, and the exponents e (N,) of the graded
    variant (read-only)."""
    rng = np.random.default_rng([seed, n, 20250829])
    b = np.stack([_sym_choice(rng, (-3, -1, 1, 3), n), _sym_choice(rng, (-2, 0, 2), n), _sym_choice(rng, (-2, 0, 2), n)])
    dm = np.stack([_sym_choice(rng, (-3, -1, 1, 3), n), _sym_choice(rng, (-5, -3, -1, 1, 3, 5), n)])
    hv = np.stack([_sym_choice(rng, range(-4, 5), n), _sym_choice(rng, range(-4, 5), n)])
    e = rng.integers(-EXP_RANGE, EXP_RANGE + 1, size=n).astype(np.float64)
    for x in (b, dm, hv, e):
        x.setflags(write=False)
    return Operands(b, dm, hv, e)


def grade(e):
    """2^(e_p + e_q) as an (N, N) matrix."""
    return np.exp2(e[:, None] + e[None, :])


def graded(ops: Operands) -> Operands:
    """The graded variant of `ops` (module docstring): same integers, inputs spanning 2^(8 EXP_RANGE)."""
    g = grade(ops.e)
    return Operands(ops.b * g, ops.dm / g, ops.hv * g, ops.e)


def dense_tensor(b):
    """(pq|rs) on the host, for the small sizes the host test compares the einsum oracles at."""
    return np.einsum("lpq,lrs->pqrs", b, b)


# ------------------------------------------------------------------------------------------ references
def jk_reference(b, dm):
    """(1 + ndm, N, N): J of the summed densities, then K per density -- the layout nbx_jk_* write."""
    dm = dm.reshape(-1, dm.shape[-1], dm.shape[-1])
    dtot = dm.sum(axis=0)
    j = np.einsum("lpq,l->pq", b, np.einsum("lrs,rs->l", b, dtot))
    k = [sum(bl @ d @ bl for bl in b) for d in dm]
    return np.stack([j] + k)


def fock_reference(b, dm, hv):
    """(fock, vhf) = (hv + J - K[x], J - K[x]) of nbx_jk_packed_fock / nbx_jk_dense_sym_fock."""
    jk = jk_reference(b, dm)
    vhf = jk[0][None] - jk[1:]
    return hv + vhf, vhf


def slab_reference(b, dm, p0: int, p1: int, convention: str):
    """(1 + ndm, N, N) additive contribution of the row slab [p0, p1) -- ("rows": (1 + ndm, p1 - p0, N)) -- in the
    convention of the kernel (module docstring): "rows", "sym", "lower" or "fold8"."""
    n = b.shape[-1]
    dm = dm.reshape(-1, n, n)
    if convention == "rows":
        return np.ascontiguousarray(jk_reference(b, dm)[:, p0:p1])
    if convention == "fold8":
        out = np.zeros((1 + dm.shape[0], n, n))
        for m, sign in ((p1, 1.0), (p0, -1.0)):
            if m > 0:
                out[:, :m, :m] += sign * jk_reference(b[:, :m, :m], dm[:, :m, :m])
        return out
    idx = np.arange(n)
    top = np.maximum(idx[:, None], idx[None, :])
    mask = ((top >= p0) & (top < p1)).astype(np.float64)
    j = jk_reference(b, dm)[0] * mask
    k = [sum((bl * mask) @ (d @ bl) for bl in b) for d in dm]
    if convention == "lower":
        k = [np.tril(x) + np.tril(x, -1).T for x in k]
    else:
        assert convention == "sym", convention
    return np.stack([j] + k)


def packed_convention(kernel: int) -> str:
    return "fold8" if kernel == M8 else "lower"


def headroom(b, dm):
    """(max over elements of the sum of |terms| of J, of K): every partial sum a kernel forms is below these."""
    dm = dm.reshape(-1, dm.shape[-1], dm.shape[-1])
    ab = np.abs(b)
    jmax = np.einsum("lpq,l->pq", ab, np.einsum("lrs,rs->l", ab, np.abs(dm).sum(axis=0))).max()
    kmax = max(sum(al @ np.abs(d) @ al for al in ab).max() for d in dm)
    return float(jmax), float(kmax)


def equal_work_cuts(n: int, parts: int = 3):
    """Row slabs [p0, p1) of equal triangular work: p(p + 1) / 2 tiles lie above row p."""
    cuts = [0] + [int(round(n * np.sqrt(i / parts))) for i in range(1, parts)] + [n]
    return [(a, c) for a, c in zip(cuts[:-1], cuts[1:]) if c > a]


def dense_slabs(n: int, limit: int = DENSE_SLAB_BYTES):
    """Row slabs whose dense form (rows x N^3 doubles) stays within `limit` bytes, as few as possible."""
    rows = max(1, limit // (8 * n ** 3))
    k = -(-n // rows)
    step = -(-n // k)
    return [(a, min(a + step, n)) for a in range(0, n, step)]


# ------------------------------------------------------------------------------------------ device-side construction
def device_rows(torch, b_dev, p0: int, p1: int):
    """Rows [p0, p1) of the dense (pq|rs) on the device from the factors (L, N, N): one fused multiply-add of outer
    products per factor -- integers (or one shared power of two per element), exact."""
    n = b_dev.shape[-1]
    out = torch.zeros((p1 - p0, n, n, n), dtype=torch.float64, device=b_dev.device)
    for bl in b_dev:
        out.addcmul_(bl[p0:p1, :, None, None], bl[None, None, :, :])
    return out


# ------------------------------------------------------------------------------------------ ao2mo
@lru_cache(maxsize=2)
def ao2mo_coefficients(case: Ao2mo, seed: int = 0):
    """C1 .. C6 (N, n_i) with entries in {+-1, +-2}: C1, C2 with n1, n2 columns, C3 / C5 with n3, C4 / C6 with n4; C1 is
    also the C12 of the pair-symmetric entry points (which need n1 == n2 to be used with C2 = C1)."""
    rng = np.random.default_rng([seed, 7, *case[:5]])
    cs = tuple(rng.choice(np.array([-2.0, -1.0, 1.0, 2.0]), size=(case.n, m))
               for m in (case.n1, case.n2, case.n3, case.n4, case.n3, case.n4))
    for c in cs:
        c.setflags(write=False)
    return cs


def ao2mo_factors(b, ca, cb):
    """(L, na, nb): Ca^T B_L Cb."""
    return np.stack([ca.T @ bl @ cb for bl in b])


def ao2mo_reference(b, c1, c2, c3, c4):
    """(n1, n2, n3, n4) on the host (small cases; the GPU test forms the same outer products on the device in chunks)."""
    return np.einsum("lij,lkm->ijkm", ao2mo_factors(b, c1, c2), ao2mo_factors(b, c3, c4))


def ao2mo_headroom(b, cs) -> float:
    """Largest sum of |terms| of an output element (the partial sums of every quarter are below it as well: each
    quarter's |terms| are bounded by sums of the same products)."""
    ab = np.abs(b)
    c1, c2, c3, c4, c5, c6 = (np.abs(c) for c in cs)
    big = 0.0
    for ca, cb in ((c3, c4), (c5, c6)):
        big = max(big, float(np.einsum("lij,lkm->l", (c1.T @ ab @ c2).max(axis=(1, 2), keepdims=True),
                                       (ca.T @ ab @ cb).max(axis=(1, 2), keepdims=True)).sum()))
    return big


def pack_rs(eri):
    """(N, N, N, N) -> (N, N, N (N + 1) / 2): (r, s <= r) at r (r + 1) / 2 + s, the layout of nbx_eri_pack_rs."""
    n = eri.shape[0]
    r, s = np.tril_indices(n)
    return np.ascontiguousarray(eri[:, :, r, s])


# ------------------------------------------------------------------------------------------ the comparison
def assert_exact(got, ref, what: str = ""):
    """Every element, every bit (NaN anywhere fails); the message names the first offending rows."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = ~(got == ref)
    if bad.any():
        where = np.argwhere(bad)
        lead = sorted({tuple(int(v) for v in w[:-1]) for w in where[:2000]})[:3]
        rows = "; ".join(f"{ix}: got {got[ix][:6]} want {ref[ix][:6]}" for ix in lead)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at {tuple(where[0])}; rows {rows}")
