"""Shared by tests/test_host_scf_kernel_cases.py (CPU) and tests/test_gpu_scf_kernels.py (MI355X): the small kernels
the SCF cycle queues (nbed_amd/csrc/elementwise.hip) -- Fock assembly, the Huzinaga operator, the energy / |dD|
scalars with the density fused into them, the device-resident DIIS, the orbital-gradient sum, the vector algebra,
the transposes and the spin-orbital scatter -- with, per operation, operands whose result is exact in float64,
real-valued operands with the rounding bound a float64 evaluation has to meet, and a table of the shapes that are
MEANT to reach every kernel instance.

Which instance a shape runs on is decided by thresholds that get retuned.  nbx_cycle_scalars_route, nbx_diis_route
and nbx_vo_sumsq_route (include/nbx.h) report the decision -- they are the functions the launchers call -- and the
tables SCALARS_TABLE, DIIS_TABLE and VO_TABLE name the instance every shape is listed for, so that a retuning which
empties a GPU test fails tests/test_host_scf_kernel_cases.py instead.

Exact operands.  Entries are integers drawn uniformly from [-2^p, 2^p] (an operand that is multiplied by 0.5 -- vhf in
the energy, kappa = 0.5 in the Huzinaga operator, half-integer coefficients -- makes half-integers of them).  Every
operation has a BUDGET(M): an upper bound, for entries of magnitude <= M, on the magnitude of every product and of
every partial sum of its result taken in ANY order; p = exact_bits(budget) is the largest p <= 25 with
budget(2^p) < 2^52.  All intermediate values are then multiples of 1/2 below 2^52 (multiples of 1/4 below 2^51
where two halves meet), i.e. float64 numbers: every summation order, with or without FMA, on the vector units or on
the matrix cores (v_mfma_f64_16x16x4 is an IEEE fma per term) gives the same bits, and float64 numpy IS the answer.
The budgets (N = matrix order, n = vector length, M = 2^p):

    fock_uhf             4 M                     h + vemb + J - K
    huzinaga_*           2 N M^2 + M             kappa (sum_k F_ik DS_kj + sum_k F_jk DS_ki) + F_ij, kappa <= 1
    trace_prod           N^2 M^2
    cycle scalars        4 N^2 M^2               |ham| <= 3.5 M (h + vhf / 2 + hz + vemb), |D - Dold|^2 <= 4 M^2
                                                 (the Dtot' table: sums of four entries, 4 M)
    dots, DIIS           n M^2                   (the Pulay matrix entries are dot products of error vectors)
    lincomb              nvec CMAX M             |coefficient| <= CMAX = 2^10, multiples of 1/2
    axpby                (|a| + |b|) M
    vo_sumsq             max(nvir nocc) M^2

The two Frobenius norms of the scalars go through sqrt: they are required within one ulp of sqrt(exact sum), the
root taken in longdouble (a correctly rounded sqrt is within half an ulp; the device's is not assumed to be).

Real-valued operands.  Entries +-10^u, u uniform in [-6, 6], signs mixed so that results cancel (gemm_cases).  The
references are evaluated in numpy.longdouble.  An output that is a sum of L terms, each the product of at most three
float64 factors (an operand, an operand, a constant such as 0.5 or kappa), accumulated in any order, fused or not,
carries on every term at most L - 1 factors (1 + d) from the additions and 3 from forming the term, |d| <= u =
eps / 2 (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1):

    |got - ref| <= gamma_(L+2) sum |terms| < (L + 4) eps sum |terms|,      eps = 2^-52,

since gamma_k = k u / (1 - k u) < (k + 2) 2 u wherever k u < 1/2.  L counts every addend of a Hamiltonian entry
(h, vhf / 2, hz, vemb: up to 4 N^2 terms in an energy) and both products of a Huzinaga entry (2 N, + 1 with F).
The squared differences of the |dD| norms are (d - dold)^2 (1 + d)^3 each: the same count.  For the norms the bound
is applied to the sum under the root: got^2, formed in longdouble, against the reference sum, with the two further
factors (1 + d) of the root inside the +4.  The density the scalars kernel makes is a length-nocc product:
(nocc + 4) eps (|C_occ| |C_occ|^T).  The bounds are derived, not measured.

DIIS.  The error vectors are integers times one power of two (diis_vectors: exact es, exact Pulay matrix H), the trial
vectors x integers; the extrapolated
vector is compared with the combination of the stored vectors formed in longdouble with the DEVICE'S OWN
coefficients, bound (nd + 4) eps sum_k |c_k x_k|.  The coefficients themselves are compared with a longdouble
Pulay solve (pulay_solve: elimination with partial pivoting, order <= 17), bound

    |c - c_ref| <= DIIS_K m kappa_2(H) eps max|c_ref|,   m = nd + 1,

and their sum is held to 1 within that same bound (it is row 0 of H c = e_0);
the form of a backward-stable solver's forward error (Higham, theorem 9.5 with the growth factor inside K).  K is
not derived: it is calibrated ON THE CPU.  Over exactly the sequences of diis_vectors(space, n, t), every space of
DIIS_SPACES, every n of DIIS_NS, space + 3 updates, numpy's float64 linalg.solve shows a worst ratio
|c - c_ref| / (m kappa_2 eps max|c_ref|) of DIIS_NUMPY_WORST_RATIO = 0.198 (space 8, n = 32768, update 9, where
kappa_2 = 4.9; the largest kappa_2 of the sequences is 2.3e3; test_host_scf_kernel_cases recomputes the ratio and fails
if it calls for a larger K); the device solves by Jacobi or by LU, both backward stable but neither numpy's
elimination, hence a factor 8: DIIS_K = the smallest power of two >= 8 x that ratio = 2.
Sequences whose vectors are shorter than nd - 1 (n = 1 with nd >= 3) have a singular Pulay matrix by construction
-- nd vectors of length n are affinely dependent -- so nothing is said about their coefficients: the stored vectors
and H are still exact.
"""

from __future__ import annotations

from functools import lru_cache

import numpy as np

EPS = float(np.finfo(np.float64).eps)
LD = np.longdouble

# ------------------------------------------------------------------------------------------ instances (include/nbx.h)
SC_REFUSED, SC_T32, SC_T16, SC_T16_DENS = range(4)      # NBX_CYCLE_SCALARS_*
SC_NAMES = {SC_REFUSED: "REFUSED", SC_T32: "T32", SC_T16: "T16", SC_T16_DENS: "T16_DENS"}
DIIS_REFUSED, DIIS_FUSED, DIIS_GENERAL = range(3)        # NBX_DIIS_*
DIIS_NAMES = {DIIS_REFUSED: "REFUSED", DIIS_FUSED: "FUSED", DIIS_GENERAL: "GENERAL"}
VO_REFUSED, VO_ONE_WG, VO_32_WG = range(3)               # NBX_VO_SUMSQ_*
VO_NAMES = {VO_REFUSED: "REFUSED", VO_ONE_WG: "ONE_WG", VO_32_WG: "32_WG"}

# the post-Fock chain: (N, (nocc_a, nocc_b)); the fused density takes 1 <= nocc <= 64 for both spins
CHAIN_FUSED = [(15, (1, 1)), (16, (3, 2)), (17, (8, 8)), (70, (63, 64)), (70, (64, 64)), (148, (40, 39)), (104, (17, 17))]
CHAIN_TWO_LAUNCH = [(70, (65, 64)), (70, (5, 0))]  # one occupied orbital too many; an empty spin
CHAIN_CASES = CHAIN_FUSED[:5] + CHAIN_TWO_LAUNCH + CHAIN_FUSED[5:]
ASYNC_T16 = [1, 15, 16, 17, 148, 496]
ASYNC_T32 = [497, 992]
SYNC_SIZES = [1, 31, 32, 33, 100, 992]  # nbx_huz_cycle_scalars: always <32>
REFUSED_SIZE = 993
DTS_SIZES = [104, 148, 117]  # with the Dtot' table (117: an odd size the packed build zero-pads)

# instance -> (nao, nocc_a, nocc_b) meant to reach it; nocc = -1: the form that is handed the density
SCALARS_TABLE = {
    SC_T16: [(n, -1, -1) for n in ASYNC_T16 + DTS_SIZES] + [(n, a, b) for n, (a, b) in CHAIN_TWO_LAUNCH],
    SC_T32: [(n, -1, -1) for n in ASYNC_T32] + [(497, 5, 5)],
    SC_T16_DENS: [(n, a, b) for n, (a, b) in CHAIN_FUSED],
    SC_REFUSED: [(REFUSED_SIZE, -1, -1), (REFUSED_SIZE, 5, 5)],
}

DIIS_SPACES = [1, 2, 6, 7, 8, 9, 16]
DIIS_NS = [1, 255, 256, 257, 2 * 37 * 37, 32768, 32769, 300001]  # 32768: the push kernel's 128 workgroups of 256
DIIS_TABLE = {
    DIIS_FUSED: [(n, nd) for n in DIIS_NS for nd in range(1, 8)],
    DIIS_GENERAL: [(n, nd) for n in DIIS_NS for nd in range(8, 17)],
    DIIS_REFUSED: [(256, 0), (256, 17), (0, 3)],
}

VO_CASES = [(5, (0, 5)), (37, (10, 9)), (148, (74, 74)), (256, (128, 127)), (257, (128, 128))]
VO_TABLE = {
    VO_ONE_WG: [(n, a, b) for n, (a, b) in VO_CASES[:4]],  # (256, (128, 127)): 128 * 128 = 16384 exactly
    VO_32_WG: [(257, 128, 128)],
    VO_REFUSED: [(5, 6, 0), (5, 0, -1), (0, 0, 0)],
}


def diis_schedule(space: int):
    """(slot, nd) of the space + 3 updates of a ring of `space` vectors: it fills, then wraps."""
    return [(t % space, min(t + 1, space)) for t in range(space + 3)]


# ------------------------------------------------------------------------------------------ exact operands
MAX_BITS = 25


def exact_bits(budget) -> int:
    """Largest p <= MAX_BITS with budget(2^p) < 2^52 (module docstring); -1 if not even p = 0 fits."""
    p = -1
    while p < MAX_BITS and budget(2 ** (p + 1)) < 2 ** 52:
        p += 1
    return p


BUDGETS = {
    "fock": lambda N: (lambda M: 4 * M),
    "huzinaga": lambda N: (lambda M: 2 * N * M * M + M),
    "trace": lambda N: (lambda M: N * N * M * M),
    "scalars": lambda N: (lambda M: 4 * N * N * M * M),
    "dots": lambda n: (lambda M: n * M * M),
    "diis": lambda n: (lambda M: n * M * M),
    "vo": lambda total: (lambda M: max(total, 1) * M * M),
}
CMAX = 2 ** 10


def lincomb_budget(nvec):
    return lambda M: nvec * CMAX * M


def ints(rng, shape, p: int):
    """Integer-valued float64 entries, uniform in [-2^p, 2^p]."""
    return rng.integers(-(2 ** p), 2 ** p + 1, size=shape).astype(np.float64)


def half_ints(rng, shape, limit: int):
    """Multiples of 1/2 in [-limit, limit] (coefficients)."""
    return rng.integers(-2 * limit, 2 * limit + 1, size=shape).astype(np.float64) / 2.0


def real_entries(rng, shape):
    """+-10^u, u uniform in [-6, 6]."""
    return rng.choice([-1.0, 1.0], size=shape) * 10.0 ** rng.uniform(-6.0, 6.0, size=shape)


def entries(kind: str, rng, shape, p: int):
    return ints(rng, shape, p) if kind == "exact" else real_entries(rng, shape)


def _freeze(*arrays):
    for x in arrays:
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return arrays


def worst_ratio(got, ref, bound) -> float:
    """max |got - ref| / bound (the difference taken in longdouble); 0 / 0 counts as 0."""
    err = np.abs(np.asarray(got, dtype=LD) - np.asarray(ref, dtype=LD)).astype(np.float64)
    bound = np.asarray(bound, dtype=np.float64)
    assert np.all(bound >= 0) and np.all(np.isfinite(bound))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.max(r)) if r.size else 0.0


def ulps_apart(got: float, want) -> float:
    """|got - want| in units of the float64 spacing at want (want: longdouble)."""
    w = float(want)
    return float(abs(LD(got) - LD(want)) / LD(np.spacing(abs(w)) if w != 0 else np.finfo(np.float64).tiny))


# ------------------------------------------------------------------------------------------ Fock assembly
@lru_cache(maxsize=4)
def fock_operands(kind: str, N: int, seed: int = 0):
    """h3 (2,N,N) (h3[0] serves as the 2-D hcore), vemb (2,N,N), jk (3,N,N)."""
    rng = np.random.default_rng([seed, N, kind == "exact", 11])
    p = exact_bits(BUDGETS["fock"](N))
    return _freeze(entries(kind, rng, (2, N, N), p), entries(kind, rng, (2, N, N), p), entries(kind, rng, (3, N, N), p))


def fock_reference(h, vemb, jk):
    """(fock, vhf, bound_fock, bound_vhf) in longdouble; h (N,N) or (2,N,N), vemb None or (2,N,N)."""
    hl, jl = np.asarray(h, dtype=LD), np.asarray(jk, dtype=LD)
    vhf = jl[0] - jl[1:]
    terms = np.abs(h) + np.abs(jk[0]) + np.abs(jk[1:])
    fock = hl + vhf
    L = 3
    if vemb is not None:
        fock = fock + np.asarray(vemb, dtype=LD)
        terms = terms + np.abs(vemb)
        L = 4
    return fock, vhf, (L + 4) * EPS * terms, (2 + 4) * EPS * (np.abs(jk[0]) + np.abs(jk[1:]))


# ------------------------------------------------------------------------------------------ Huzinaga operator
HUZ_SIZES = [1, 15, 16, 17, 79, 80, 81, 160, 161, 241]  # the fused kernel's k range goes in trips of 80


@lru_cache(maxsize=4)
def huz_operands(kind: str, N: int, batch: int, seed: int = 0):
    """F, DS (batch,N,N)."""
    rng = np.random.default_rng([seed, N, batch, kind == "exact", 12])
    p = exact_bits(BUDGETS["huzinaga"](N))
    return _freeze(entries(kind, rng, (batch, N, N), p), entries(kind, rng, (batch, N, N), p))


def matmul_ld(a, b):
    """Batched a @ b in longdouble (numpy's object-free loop: fine at these sizes)."""
    return np.matmul(np.asarray(a, dtype=LD), np.asarray(b, dtype=LD))


def huz_fused_reference(f, ds, kappa: float):
    """(hz, fock + hz, bound_hz, bound_fock) for hz = -kappa (F DS + (F DS)^T)."""
    N = f.shape[-1]
    t = matmul_ld(f, ds)
    hz = -LD(kappa) * (t + np.swapaxes(t, -1, -2))
    ta = np.matmul(np.abs(f), np.abs(ds))
    terms = abs(kappa) * (ta + np.swapaxes(ta, -1, -2))
    return hz, np.asarray(f, dtype=LD) + hz, (2 * N + 4) * EPS * terms, (2 * N + 1 + 4) * EPS * (terms + np.abs(f))


def huz_sym_reference(fds, kappa: float, fock=None):
    """(hz, fock + hz or None, bound_hz, bound_fock or None) for hz = -kappa (FDS + FDS^T)."""
    fl = np.asarray(fds, dtype=LD)
    hz = -LD(kappa) * (fl + np.swapaxes(fl, -1, -2))
    terms = abs(kappa) * (np.abs(fds) + np.swapaxes(np.abs(fds), -1, -2))
    if fock is None:
        return hz, None, (2 + 4) * EPS * terms, None
    return hz, np.asarray(fock, dtype=LD) + hz, (2 + 4) * EPS * terms, (3 + 4) * EPS * (terms + np.abs(fock))


# ------------------------------------------------------------------------------------------ traces and the cycle's scalars
TRACE_SIZES = [1, 31, 32, 33, 2016]
TRACE_REFUSED = 2017


@lru_cache(maxsize=2)
def trace_operands(kind: str, N: int, seed: int = 0):
    rng = np.random.default_rng([seed, N, kind == "exact", 13])
    p = exact_bits(BUDGETS["trace"](N))
    return _freeze(entries(kind, rng, (2, N, N), p), entries(kind, rng, (2, N, N), p))


def trace_reference(a, b):
    """(sum_ij A_ij B_ji per batch entry in longdouble, bound)."""
    N = a.shape[-1]
    bt = np.swapaxes(b, -1, -2)
    ref = np.sum(np.asarray(a, dtype=LD) * np.asarray(bt, dtype=LD), axis=(-2, -1))
    return ref, (N * N + 4) * EPS * np.sum(np.abs(a) * np.abs(bt), axis=(-2, -1))


@lru_cache(maxsize=3)
def scalars_operands(kind: str, N: int, seed: int = 0):
    """h3 (2,N,N) (h3[0] also serves as a 2-D hcore), vemb, vhf, hz, dm, dm_old (2,N,N): six unrelated matrices."""
    rng = np.random.default_rng([seed, N, kind == "exact", 14])
    p = exact_bits(BUDGETS["scalars"](N))
    return _freeze(*(entries(kind, rng, (2, N, N), p) for _ in range(6)))


def scalars_reference(h, vemb, vhf, hz, dm, dm_old):
    """The four scalars of a cycle.  Returns (energy (2,) longdouble, bound (2,), sumsq (2,) longdouble, bound (2,)):
    energy[x] = sum_ij (h + vhf / 2 + hz + vemb)[x][i,j] D[x][j,i]; sumsq[x] = sum (D - Dold)[x]^2 (the kernel
    reports its square root).  h (N,N) or (2,N,N); vemb, hz may be None."""
    N = dm.shape[-1]
    dt = np.swapaxes(dm, -1, -2)
    ham = np.asarray(h, dtype=LD) + LD(0.5) * np.asarray(vhf, dtype=LD)
    aham = np.abs(h) + 0.5 * np.abs(vhf)
    addends = 2
    for extra in (hz, vemb):
        if extra is not None:
            ham = ham + np.asarray(extra, dtype=LD)
            aham = aham + np.abs(extra)
            addends += 1
    ham = np.broadcast_to(ham, dm.shape)
    energy = np.sum(ham * np.asarray(dt, dtype=LD), axis=(-2, -1))
    e_bound = (addends * N * N + 4) * EPS * np.sum(np.broadcast_to(aham, dm.shape) * np.abs(dt), axis=(-2, -1))
    dd = np.asarray(dm, dtype=LD) - np.asarray(dm_old, dtype=LD)
    sumsq = np.sum(dd * dd, axis=(-2, -1))
    return energy, e_bound, sumsq, (N * N + 4) * EPS * sumsq.astype(np.float64)


def check_scalars(got, ref, exact: bool):
    """Assert the four scalars `got` against scalars_reference's `ref`; returns the worst error / bound (0 if exact)."""
    energy, e_bound, sumsq, s_bound = ref
    got = np.asarray(got, dtype=np.float64)
    if exact:
        np.testing.assert_array_equal(got[:2], energy.astype(np.float64))
        assert all(LD(float(e)) == e for e in energy)  # (the reference itself was exact)
        for x in range(2):
            assert ulps_apart(got[2 + x], np.sqrt(sumsq[x])) <= 1.0, (x, got[2 + x], np.sqrt(sumsq[x]))
        return 0.0
    worst = max(worst_ratio(got[:2], energy, e_bound), worst_ratio(np.asarray(got[2:], dtype=LD) ** 2, sumsq, s_bound))
    assert worst <= 1.0, (worst, got, energy, np.sqrt(sumsq))
    return worst


def dts_restatement(dm):
    """What the scalars kernel leaves per pair a >= b for the next packed J/K build: sum_x (D_ab + D_ba) below the
    diagonal, sum_x D_aa on it.  (N,N), the upper triangle zero."""
    tot = dm[0] + dm[1]
    low = np.tril(tot + tot.T, -1)
    return low + np.diag(np.diag(tot))


def dts_layout(N: int):
    """Where the Dtot' table of a size the 8-fold packed kernel has an instance for (N = 4 NB: 104 and 148 here) keeps
    the pair (row, col <= row): csrc/jk_m8_layout.h and m4_weight_index_rt of csrc/jk_m4_layout.h restated.  The
    density is cut into 4 x 4 blocks (bt, bc) = (row // 4, col // 4); the block rows of the lower triangle are
    filled greedily into chunks of at most 32 LP blocks, LP the smallest count that gives at most four chunks;
    chunk k starts at k LP 512 doubles, the blocks of a chunk follow each other in row-major triangle order, 16
    doubles each, swizzled inside: 4 (kk ^ ((bt ^ bc) & 3)) + (ii ^ kk) with (ii, kk) = (row % 4, col % 4).
    Returns (index (N, N) int64 with -1 above the diagonal, table length in doubles)."""
    assert N % 4 == 0
    NB = N // 4

    def tri(k):
        return k * (k + 1) // 2

    def chunk_rows(lp):
        rows, r = [], 0
        while r < NB:
            rows.append(r)
            blk = 0
            while r < NB and blk + r + 1 <= 32 * lp:
                r += 1
                blk += r
        return rows

    lp = (NB + 1 + 31) // 32
    while len(chunk_rows(lp)) > 4:
        lp += 1
    starts = chunk_rows(lp)
    assert len(starts) <= 4
    row, col = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    bt, bc, ii, kk = row >> 2, col >> 2, row & 3, col & 3
    k = np.searchsorted(np.array(starts), bt, side="right") - 1
    rk = np.array(starts)[k]
    idx = k * lp * 512 + 16 * (tri(bt) + bc - tri(rk)) + 4 * (kk ^ ((bt ^ bc) & 3)) + (ii ^ kk)
    return np.where(col <= row, idx, -1).astype(np.int64), len(starts) * lp * 512


def density_reference(c, nocc):
    """(D longdouble, bound) for D[x] = C[x][:, :nocc_x] C[x][:, :nocc_x]^T from the given (device-made) orbitals."""
    d = np.zeros(c.shape, dtype=LD)
    bound = np.zeros(c.shape)
    for x in range(c.shape[0]):
        k = int(nocc[x])
        co = c[x][:, :k]
        d[x] = matmul_ld(co, co.T)
        bound[x] = (k + 4) * EPS * (np.abs(co) @ np.abs(co).T)
    return d, bound


@lru_cache(maxsize=2)
def chain_operands(N: int, seed: int = 0):
    """The post-Fock chain on a chosen J/K: integer hv (2,N,N), jk (3,N,N), ds (2,N,N), dm_in (2,N,N) with the
    Huzinaga budget (Fock entries reach 3 M: the budget is taken at 3 M), and a real SPD overlap S with X = S^-1/2."""
    rng = np.random.default_rng([seed, N, 15])
    p = exact_bits(lambda M: BUDGETS["huzinaga"](N)(3 * M))
    p = min(p, 6)  # (small integers keep the Fock spectrum well separated from rounding: the eigensolver is not under test)
    hv0 = ints(rng, (2, N, N), p)
    hv = hv0 + np.swapaxes(hv0, -1, -2) - 40.0 * N * np.eye(N) * np.arange(1, 3)[:, None, None]
    jk0 = ints(rng, (3, N, N), p)
    jk = jk0 + np.swapaxes(jk0, -1, -2)
    ds = np.zeros((2, N, N))
    ds[:, :, : max(1, N // 8)] = ints(rng, (2, N, max(1, N // 8)), min(p, 2))  # (a low-rank environment projector's shape)
    dm_in = ints(rng, (2, N, N), p)
    g = rng.standard_normal((N, N))
    s = np.eye(N) + 0.3 * (g @ g.T) / N
    s = 0.5 * (s + s.T)
    w, v = np.linalg.eigh(s)
    x = (v / np.sqrt(w)) @ v.T
    return _freeze(hv, jk, ds, dm_in, s, 0.5 * (x + x.T))


MU_CASES = [(16, (3, 2)), (17, (8, 8)), (70, (30, 29))]
MU_SPACE, MU_CYCLES = 8, 10  # CDIIS keeps 8 vectors: ten cycles wrap the ring


@lru_cache(maxsize=2)
def mu_operands(N: int, seed: int = 0):
    """The mu-shift chain: integer h1e (2,N,N) and J/K (3,N,N), symmetric; an INTEGER overlap S = 2 N I + E with E
    symmetric in {-1, 0, 1} (diagonally dominant, so positive definite) and X = S^-1/2."""
    rng = np.random.default_rng([seed, N, 23])
    h0, jk0 = ints(rng, (2, N, N), 6), ints(rng, (3, N, N), 6)
    e = np.triu(ints(rng, (N, N), 0), 1)
    s = 2.0 * N * np.eye(N) + e + e.T
    w, v = np.linalg.eigh(s)
    x = (v / np.sqrt(w)) @ v.T
    return _freeze(h0 + np.swapaxes(h0, -1, -2), jk0 + np.swapaxes(jk0, -1, -2), s, 0.5 * (x + x.T))


MU_BITS = 8


def mu_cycle_inputs(N: int, t: int, seed: int = 0):
    """(D_t, F_t): the symmetric integer density and Fock matrix cycle t is handed.  With |S| <= 2 N + 1 and entries
    up to 2^(MU_BITS + 1), every partial sum of (S D F)^T - S D F stays below 2 N^2 (2 N + 1) 4^(MU_BITS + 1) < 2^52:
    the CDIIS error vector is exact."""
    assert 2 * N * N * (2 * N + 1) * 4 ** (MU_BITS + 1) < 2 ** 52
    rng = np.random.default_rng([seed, N, t, 24])
    d0, f0 = ints(rng, (2, N, N), MU_BITS), ints(rng, (2, N, N), MU_BITS)
    return d0 + np.swapaxes(d0, -1, -2), f0 + np.swapaxes(f0, -1, -2) - 8.0 * N * np.eye(N)


def grad_reference(c, fock, nocc):
    """The orbital-gradient sums g[x] = sum_{a >= nocc, i < nocc} (C^T F C)[x][a,i]^2 from the given orbitals and Fock
    matrix.  The device forms f = (C^T F) C by two products of length N: |f_ai - ref_ai| <= d_ai = (2 N + 4) eps
    (|C|^T |F| |C|)_ai (the inner product's error passes through the outer one: gamma_N + gamma_N + their product
    < (2 N + 4) eps), and the sum of L = nvir nocc squares adds (L + 4) eps sum f^2:
    |g - g_ref| <= sum (2 |ref_ai| d_ai + d_ai^2) + (L + 4) eps sum (|ref_ai| + d_ai)^2."""
    N = c.shape[-1]
    ref, bound = np.zeros(2, dtype=LD), np.zeros(2)
    for x, k in enumerate(nocc):
        f = matmul_ld(matmul_ld(c[x].T, fock[x]), c[x])[k:, :k]
        d = (2 * N + 4) * EPS * (np.abs(c[x]).T @ np.abs(fock[x]) @ np.abs(c[x]))[k:, :k]
        fa = np.abs(f).astype(np.float64)
        ref[x] = np.sum(f * f)
        bound[x] = np.sum(2 * fa * d + d * d) + ((N - k) * k + 4) * EPS * np.sum((fa + d) ** 2)
    return ref, bound


# ------------------------------------------------------------------------------------------ vector algebra
VEC_NS = [1, 255, 256, 257, 32768, 32769]
VEC_NVECS = [1, 5, 16]
VEC_NVEC_REFUSED = 17
PAST_GRID_N = 65536 * 256 + 257  # one element more than a whole grid of 65536 x 256 passes over, and an odd tail


@lru_cache(maxsize=2)
def vec_operands(kind: str, n: int, nvec: int, seed: int = 0):
    """x (n,), vecs (nvec, n), coefficients (nvec,) (half-integers up to CMAX, or real)."""
    rng = np.random.default_rng([seed, n, nvec, kind == "exact", 16])
    p = min(exact_bits(BUDGETS["dots"](n)), exact_bits(lincomb_budget(nvec)))
    coef = half_ints(rng, nvec, CMAX) if kind == "exact" else real_entries(rng, nvec)
    return _freeze(entries(kind, rng, n, p), entries(kind, rng, (nvec, n), p), coef)


def dots_reference(x, vecs):
    ref = np.sum(np.asarray(vecs, dtype=LD) * np.asarray(x, dtype=LD), axis=-1)
    return ref, (x.size + 4) * EPS * (np.abs(vecs) @ np.abs(x))


def lincomb_reference(coef, vecs):
    c = np.asarray(coef, dtype=LD)[:, None]
    ref = np.sum(c * np.asarray(vecs, dtype=LD), axis=0)
    return ref, (len(coef) + 4) * EPS * np.sum(np.abs(np.asarray(coef, dtype=np.float64))[:, None] * np.abs(vecs), axis=0)


def axpby_reference(a, x, b, y):
    ref = LD(a) * np.asarray(x, dtype=LD) + LD(b) * np.asarray(y, dtype=LD)
    return ref, (2 + 4) * EPS * (abs(a) * np.abs(x) + abs(b) * np.abs(y))


# ------------------------------------------------------------------------------------------ orbital-gradient sum
@lru_cache(maxsize=2)
def vo_operands(kind: str, N: int, nocc, seed: int = 0):
    """fmo (2,N,N): the virtual-occupied block [nocc_x:, :nocc_x] of spin x holds the operands, everything else NaN."""
    rng = np.random.default_rng([seed, N, nocc[0], nocc[1], kind == "exact", 17])
    total = max((N - k) * k for k in nocc)
    p = exact_bits(BUDGETS["vo"](total))
    fmo = np.full((2, N, N), np.nan)
    for x, k in enumerate(nocc):
        fmo[x, k:, :k] = entries(kind, rng, (N - k, k), p)
    return _freeze(fmo)[0]


def vo_reference(fmo, nocc):
    ref = np.array([np.sum(np.asarray(fmo[x, k:, :k], dtype=LD) ** 2) for x, k in enumerate(nocc)], dtype=LD)
    L = np.array([(fmo.shape[-1] - k) * k for k in nocc])
    return ref, (L + 4) * EPS * ref.astype(np.float64)


# ------------------------------------------------------------------------------------------ spin-orbital scatter
def spinorb_restatement(one_body, two_body, tol: float, scale: float):
    """nbed/ham_builder.py:180-214 in numpy: the spatial blocks interleaved into spin orbitals, |x| < tol zeroed,
    the two-body part scaled."""
    n = one_body.shape[-1]
    h1 = np.zeros((2 * n,) * 2)
    h2 = np.zeros((2 * n,) * 4)
    h1[0::2, 0::2] = one_body[0]
    h1[1::2, 1::2] = one_body[1]
    h2[0::2, 0::2, 0::2, 0::2] = two_body[0]
    h2[1::2, 1::2, 1::2, 1::2] = two_body[1]
    h2[0::2, 1::2, 1::2, 0::2] = two_body[2]
    h2[1::2, 0::2, 0::2, 1::2] = two_body[3]
    h1[np.abs(h1) < tol] = 0.0
    h2[np.abs(h2) < tol] = 0.0
    return h1, h2 * scale


@lru_cache(maxsize=2)
def spinorb_operands(n: int, tol: float, seed: int = 0):
    """one_body (2,n,n), two_body (4,n,n,n,n): real entries of every size around `tol`, among them exactly +-tol
    (kept) and the float64 numbers next below in magnitude (zeroed)."""
    rng = np.random.default_rng([seed, n, 18])
    below = np.nextafter(tol, 0.0)
    special = np.array([tol, -tol, below, -below, 0.0, -0.0])
    out = []
    for shape in ((2, n, n), (4, n, n, n, n)):
        v = rng.choice([-1.0, 1.0], size=shape) * tol * 10.0 ** rng.uniform(-3.0, 3.0, size=shape)
        pick = rng.random(shape) < 0.3
        v[pick] = rng.choice(special, size=int(pick.sum()))
        k = min(special.size, v.size)  # (every one of them at least once where there is room; the last element -tol)
        v.reshape(-1)[np.linspace(0, v.size - 1, k).astype(int)] = special[:k]
        v.reshape(-1)[-1] = -tol
        out.append(v)
    return _freeze(*out)


# ------------------------------------------------------------------------------------------ DIIS
def diis_bits_and_shift(n: int):
    """(p, s): the error vectors of length n are integers of [-2^p, 2^p] times 2^-s."""
    p = min(exact_bits(BUDGETS["diis"](n)), 12)
    return p, int(round(0.5 * np.log2(n * 4.0 ** p / 3.0)))


def diis_vectors(space: int, n: int, t: int, seed: int = 0):
    """(x_t, err_t): the trial and error vector of update t of the sequence (space, n).  x_t: integers.  err_t:
    integers times ONE power of two, 2^-s with 4^s ~ n 4^p / 3 -- still exact (every product and sum is an integer
    multiple of 4^-s within the budget), and <e, e> ~ 1, so that the Pulay matrix, bordered by ones, is not
    ill-conditioned by a mere mismatch of scale: the coefficient bound, proportional to kappa_2(H), stays sharp."""
    rng = np.random.default_rng([seed, space, n, t, 19])
    p, s = diis_bits_and_shift(n)
    return ints(rng, n, p), ints(rng, n, p) * 2.0 ** -s


def pulay_matrix(space: int):
    h = np.zeros((space + 1, space + 1))
    h[0, 1:] = h[1:, 0] = 1.0
    return h


def pulay_solve(h):
    """Solve H c = e_0 in longdouble by Gaussian elimination with partial pivoting; returns c (all m entries)."""
    a = np.array(h, dtype=LD)
    m = a.shape[0]
    assert a.shape == (m, m) and m <= 17
    b = np.zeros(m, dtype=LD)
    b[0] = 1
    for k in range(m):
        piv = k + int(np.argmax(np.abs(a[k:, k])))
        if piv != k:
            a[[k, piv]] = a[[piv, k]]
            b[[k, piv]] = b[[piv, k]]
        for i in range(k + 1, m):
            f = a[i, k] / a[k, k]
            a[i, k:] -= f * a[k, k:]
            b[i] -= f * b[k]
    c = np.zeros(m, dtype=LD)
    for i in range(m - 1, -1, -1):
        c[i] = (b[i] - np.dot(a[i, i + 1:], c[i + 1:])) / a[i, i]
    return c


DIIS_NUMPY_WORST_RATIO = 0.198
DIIS_K = 2.0


def diis_k_from_ratio(ratio: float) -> float:
    """The smallest power of two >= 8 x ratio."""
    return float(2.0 ** np.ceil(np.log2(8.0 * ratio)))


def diis_coef_bound(h_sub, c_ref) -> float:
    """DIIS_K m kappa_2(H) eps max|c_ref| for the (nd + 1) x (nd + 1) Pulay system (c_ref: all m entries or c[1:])."""
    m = h_sub.shape[0]
    return DIIS_K * m * float(np.linalg.cond(h_sub, 2)) * EPS * float(np.max(np.abs(np.asarray(c_ref, dtype=np.float64))))


def diis_singular_by_construction(n: int, nd: int) -> bool:
    """nd error vectors of length n < nd - 1 are affinely dependent: the bordered Gram matrix is singular."""
    return n < nd - 1


class DiisHost:
    """The host's float64 copy of a ring: stored vectors and the Pulay matrix, exact for integer vectors."""

    def __init__(self, space: int, n: int):
        self.space, self.n = space, n
        self.xs, self.es = np.zeros((space, n)), np.zeros((space, n))
        self.h = pulay_matrix(space)

    def push(self, slot: int, nd: int, x, e):
        self.xs[slot], self.es[slot] = x, e
        row = self.es[:nd] @ e
        self.h[slot + 1, 1:nd + 1] = row
        self.h[1:nd + 1, slot + 1] = row
        return self.h[:nd + 1, :nd + 1]

    def extrapolate(self, coef, nd: int):
        """(sum_k c_k xs[k] in longdouble, bound) with the given coefficients."""
        c = np.asarray(coef[:nd], dtype=LD)[:, None]
        ref = np.sum(c * np.asarray(self.xs[:nd], dtype=LD), axis=0)
        bound = (nd + 4) * EPS * np.sum(np.abs(np.asarray(coef[:nd], dtype=np.float64))[:, None] * np.abs(self.xs[:nd]), axis=0)
        return ref, bound


# ------------------------------------------------------------------------------------------ transposes
TRANSPOSE_SHAPES = [(1, 1), (31, 33), (32, 32), (33, 31), (1, 300), (300, 1)]
TRANSPOSE_TWO_CHUNKS = (4, 4, 70000)  # rows, cols, batch: a grid's z extent ends at 65535
