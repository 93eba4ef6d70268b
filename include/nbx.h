/*
 * nbx.h -- C ABI of libnbx: MI355X (gfx950) kernels for the embedded-SCF hot
 * path of UCL-CCS/Nbed (Huzinaga / mu-shift Fock build, J/K contraction,
 * projector products, symmetric eigensolve, SPADE / concentric-localisation
 * SVDs, AO->active-MO four-index transform, spin-orbital scatter).
 *
 * The reference is pure Python and has no FFI of its own; what this library
 * replaces are the calls the reference makes into PySCF's C libraries and
 * into NumPy/SciPy LAPACK on that path.  Each entry point cites the reference
 * call site(s) it stands in for (paths relative to the reference repository).
 *
 * Conventions (binding):
 *   - extern "C", every function returns int: 0 = ok, < 0 = error
 *     (NBX_E_*); nbx_last_error() returns a thread-local message.
 *   - No exceptions cross the boundary.  Caller allocates every output.
 *   - Matrices are row-major (C order) double precision.  "d_" pointers are
 *     DEVICE pointers (hipMalloc / nbx_malloc / torch tensor data_ptr);
 *     "h_" pointers are host pointers.
 *   - Sizes are int64_t.  Work runs asynchronously on the context's HIP
 *     stream; nbx_sync() or a d2h copy waits for it.
 *   - A context is bound to one device and one stream and must not be used
 *     from two threads at once; the library keeps no other global state.
 *   - Multi-GPU: one process (context) per GPU.  Entry points that shard take
 *     an index range [i0, i1) and compute that slab only; the exchange step
 *     (all-gather over RCCL) is done by the host (torch.distributed).
 */
#ifndef NBX_H
#define NBX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version: bumped whenever the meaning or the size of a buffer behind an existing entry point changes (a caller
 * built against an older header would otherwise get silent out-of-bounds writes, not an error).  Callers compare
 * nbx_version() with the NBX_VERSION they were built against and refuse to run on a mismatch (nbed_amd/_nbx.py does).
 *   2 (round 4): nbx_huz_cycle's h_out is 7 doubles (was 6); nbx_huz_cycle_scalars_dev/_dts write a ready word at
 *     d_out[4 + tail_n]; nbx_diis_update*'s d_coef holds nbx_diis_coef_doubles(space) zeroed doubles; nbx_huz_state
 *     gained jk_kind, jk_p0, jk_p1, d_eri and (jk_p0, jk_p1) = (0, 0) now means an EMPTY slab; nbx_xc_density /
 *     nbx_xc_half are gone; nbx_mu_cycle* are new.
 *   3 (round 4): the packed tensor of N = 97 .. 148 is the 8-fold form (nbx_eri_packed_bytes / nbx_jk_packed_worksize /
 *     nbx_jk_dts_bytes return other sizes for it: a packed buffer kept from a version-2 library is not this one's);
 *     nbx_jk_packed_fold and nbx_sym_pow_ns* are new; nbx_eigh_tridiag_worksize grew by one status slot.          */
#define NBX_VERSION 3

#define NBX_OK 0
#define NBX_E_INVALID (-1)  /* bad argument (null pointer, negative size, shape mismatch) */
#define NBX_E_HIP (-2)      /* a HIP runtime call failed (message has the HIP error string) */
#define NBX_E_NOMEM (-3)    /* workspace too small / allocation failed */
#define NBX_E_NOCONV (-4)   /* iterative kernel hit its sweep limit (results still written) */
#define NBX_E_UNSUPPORTED (-5)
#define NBX_E_INTERNAL (-6) /* a consistency check of the library on its own tables failed (a bug: the message says which) */

typedef struct nbx_ctx nbx_ctx;

/* ------------------------------------------------------------------ context */
int nbx_version(void);
const char* nbx_last_error(void);
int nbx_device_count(int* count);
/* stream: the hipStream_t to launch on (e.g. torch's current stream; NULL = the device's
 * default stream).  private_stream != 0: ignore `stream` and create a private non-blocking
 * stream owned by the context. */
int nbx_ctx_create(int device, void* stream, int private_stream, nbx_ctx** ctx);
int nbx_ctx_destroy(nbx_ctx* ctx);
int nbx_ctx_set_stream(nbx_ctx* ctx, void* stream);
int nbx_sync(nbx_ctx* ctx);
int nbx_malloc(nbx_ctx* ctx, size_t bytes, void** d_ptr);
int nbx_free(nbx_ctx* ctx, void* d_ptr);
int nbx_memcpy_h2d(nbx_ctx* ctx, void* d_dst, const void* h_src, size_t bytes);
int nbx_memcpy_d2h(nbx_ctx* ctx, void* h_dst, const void* d_src, size_t bytes); /* synchronises */
/* count <= 8 device arrays of doubles, one after the other, into h_dst: PINNED (device-mapped) host memory the
 * kernel stores to directly -- one launch (the results of an SCF run).  h_dst: sum(n_doubles) + 1 doubles; the
 * last one receives 1.0 once everything before it is visible to the host.  wait != 0: synchronises the stream;
 * wait = 0: returns after the launch -- the caller cleared that word beforehand and polls it. */
int nbx_gather_to_host(nbx_ctx* ctx, int64_t count, const double* const* d_src, const int64_t* n_doubles,
                       double* h_dst, int wait);
int nbx_memcpy_d2d(nbx_ctx* ctx, void* d_dst, const void* d_src, size_t bytes);
int nbx_memset(nbx_ctx* ctx, void* d_ptr, int value, size_t bytes);

/* ------------------------------------------------------------------ density-fitted J/K (an extra)
 * (pq|rs) ~ sum_L B_L[p][q] B_L[r][s] with symmetric B_L -- what PySCF contracts
 * behind get_veff (huzinaga_scf.py:156, driver.py:344,847) when the mean-field object is built with
 * .density_fit().  The reference never asks for that; this entry point is NOT on the parity path of the exact
 * integrals.  It is the GEMM-shaped form of J/K, the only one there is at N_AO = 2000:
 *   J = sum_L B_L <B_L, D_a + D_b>,   K^x = sum_L (B_L C^x)(B_L C^x)^T,   D^x = C^x C^x^T.
 * d_b: (naux, N, N) the auxiliary functions this rank holds (results are additive over slabs of L);
 * d_c: (ndm, N, N) orbital coefficients whose first nocc[x] COLUMNS are the occupied orbitals of spin x
 *      (ndm = 1: closed shell, D_a = D_b); d_jk: (1 + ndm, N, N) = J, K_a[, K_b].
 * nbx_df_synth: d_b[l - l0][p][q] = scale * val(stream 9, l N(N+1)/2 + tri(p, q)), l in [l0, l1).               */
size_t nbx_jk_df_worksize(int64_t nao, int64_t ndm, int64_t nocc_max);
int nbx_jk_df(nbx_ctx* ctx, int64_t nao, int64_t naux, const double* d_b, int64_t ndm, const double* d_c,
              const int64_t* nocc, double* d_jk, void* d_work, size_t work_bytes);
int nbx_df_synth(nbx_ctx* ctx, int64_t nao, int64_t l0, int64_t l1, uint64_t seed, double scale, double* d_b);

/* ------------------------------------------------------------------ in-library kernel timing
 * While enabled, the listed launches are bracketed by HIP events recorded on the context's
 * stream; nbx_profile_read() waits for them and returns the accumulated milliseconds and
 * launch count of a slot.  bench.py uses this for the roofline numbers.                    */
#define NBX_PROF_JK_DENSE 0    /* jk_dense_kernel (the streaming kernel of nbx_jk_dense)     */
#define NBX_PROF_AO2MO_Q1 1    /* first quarter-transform GEMM of nbx_ao2mo                  */
#define NBX_PROF_AO2MO 2       /* all four quarter transforms of one nbx_ao2mo call          */
#define NBX_PROF_EIGH 3        /* eigh_jacobi_kernel                                         */
#define NBX_PROF_SVD 4         /* svd_jacobi_kernel                                          */
#define NBX_PROF_GEMM 5        /* every gemm_f64_kernel launch                               */
#define NBX_PROF_LOC 6         /* loc_pm_kernel / loc_boys_kernel                            */
/* (7 = NBX_PROF_ERI: the class launches of nbx_eri_device, read with nbx_eri_class_ms)                  */
/* on = 0: off; on = 1: every slot; on = 2 | (mask << 2): only the slots whose bit is set in
 * mask (an event pair costs a few microseconds of stream time, which matters inside an SCF
 * cycle: bench.py brackets the J/K kernel only).                                             */
int nbx_profile_enable(nbx_ctx* ctx, int on);
/* Bracket only one launch in `every` of each enabled slot (the first after nbx_profile_reset, then every
 * `every`-th; default 1 = all of them).  An event pair holds the stream for ~11 us (two marker packets of ~6 us
 * each, measured on a rocprofv3 kernel trace with and without them: profiles/r03/README.md), 4 % of a settled
 * N_AO = 148 cycle: bench.py samples the J/K launch of every fourth cycle of its timed region.           */
int nbx_profile_sample(nbx_ctx* ctx, int every);
/* Test support: fills the LDS of every CU with `value` (tests pass a NaN) so that a kernel reading LDS it has not
 * written fails its parity test instead of depending on what ran on the CU before (tests/test_gpu_kernels.py).   */
int nbx_debug_fill_lds(nbx_ctx* ctx, double value);
int nbx_profile_read(nbx_ctx* ctx, int slot, double* ms_sum, int64_t* count);
int nbx_profile_reset(nbx_ctx* ctx);

/* ------------------------------------------------------------------ synthetic inputs
 * Counter-hash (pq|rs) of SURVEY.md section 8d, rows p in [p0,p1) of the dense
 * C-order (N,N,N,N) tensor: d_eri[(p-p0),q,r,s] = val(canon(p,q,r,s)) / N.
 * Stands in for mol.intor('int2e') (reached through PySCF get_veff / ao2mo.kernel,
 * nbed/scf/huzinaga_scf.py:156, nbed/ham_builder.py:128). */
int nbx_synth_eri(nbx_ctx* ctx, int64_t nao, int64_t p0, int64_t p1, uint64_t seed, double* d_eri);

/* ------------------------------------------------------------------ J/K contraction
 * Replaces PySCF UHF.get_jk / get_veff (libcvhf) at nbed/scf/huzinaga_scf.py:156,
 * nbed/scf/embedded_hcore_funcs.py:34, nbed/driver.py:344-345,847-849,
 * nbed/localizers/virtual/concentric.py:104,109.
 *   d_eri : slab rows p in [p0,p1) of the dense (N,N,N,N) chemist-order ERI
 *   d_dm  : (ndm,N,N) density matrices (ndm = 1 or 2), symmetric
 *   d_jk  : out, ((1+ndm), p1-p0, N):  [0] = J rows from sum_x dm[x],
 *           [1+x] = K rows from dm[x]:  J_pq = sum_rs (pq|rs) D_rs,
 *           K_pr = sum_qs (pq|rs) D_qs   (uses (pq|rs) = (pq|sr))
 *   d_work: nbx_jk_dense_worksize() bytes                                  */
size_t nbx_jk_dense_worksize(int64_t nao, int64_t np, int64_t ndm);
int nbx_jk_dense(nbx_ctx* ctx, int64_t nao, int64_t p0, int64_t p1, const double* d_eri,
                 const double* d_dm, int64_t ndm, double* d_jk, void* d_work, size_t work_bytes);

/* Symmetric form: (pq|rs) = (qp|rs), so only the tiles q <= p of the slab are read -- half the
 * bytes of nbx_jk_dense, which is HBM bound (PySCF's libcvhf, which the reference calls, works on
 * 8-fold packed integrals).  The interface is ADDITIVE over slabs:
 *   d_jk : out, ((1+ndm), N, N) full-size matrices holding the contribution of slab rows
 *          p in [p0,p1): all pairs (p, q <= p) and their mirror images; [0] = J, [1+x] = K of
 *          dm[x].  With p0 = 0, p1 = N they are the result; across GPUs the slabs' outputs are
 *          summed (all-reduce).  The work of a slab grows with p: equal-work slabs are not
 *          equal-height.
 * Sizes the symmetric kernel does not cover (odd N, N > 512) go through nbx_jk_dense inside.  */
size_t nbx_jk_dense_sym_worksize(int64_t nao, int64_t p0, int64_t p1, int64_t ndm);
int nbx_jk_dense_sym(nbx_ctx* ctx, int64_t nao, int64_t p0, int64_t p1, const double* d_eri,
                     const double* d_dm, int64_t ndm, double* d_jk, void* d_work, size_t work_bytes);

/* Packed form: (pq|rs) = (qp|rs) = (pq|sr), so only q <= p and s <= r are stored and read -- a
 * quarter of the dense tensor (PySCF holds `mf._eri` 8-fold packed and libcvhf, which the
 * reference reaches through get_veff at nbed/scf/huzinaga_scf.py:156, contracts it packed).
 * nbx_eri_pack converts slab rows [p0,p1) of the dense tensor ONCE (the integrals do not change
 * during an SCF); nbx_jk_packed then reads nbx_eri_packed_bytes() per call instead of
 * 8 N^4 (p1-p0)/N.  Storage: the tiles T(p,q) = p(p+1)/2 + q, q <= p, in sequence; a tile is the
 * lower triangle of its (r,s) matrix cut into NB = 2 (N <= 128) or 4 blocks of s = N/NB rows:
 * first the NB diagonal triangles (row-major, packed), then for r = 1..NB-1 the rectangles
 * (I, J = I ^ r), I > J, ordered by the row block I, row-major with row stride s|1 (zero pad); each
 * of the NB chunks padded to an even number of doubles.
 * N = 100, 104, ..., 148 have a layout and a kernel of their own (csrc/jk_m4.hip, one instance per size, the contraction on
 * v_mfma_f64_4x4x4_4b_f64; N = 97 .. 147 that are not multiples of four run as the next multiple with the extra rows and
 * columns zero -- the padding is internal, as for jk_s4.hip's padded sizes): a tile is the
 * lower triangle in 4 x 4 blocks, block (T, C <= T) at T(T+1)/2 + C, element (i, k) at 4 (k ^ ((T ^ C) & 3)) + (i ^ k),
 * zeros above the diagonal of the diagonal blocks; NBX_JK_M4=0 in the environment keeps the layout above.  Either way the
 * packed buffer is opaque to the caller: nbx_eri_packed_bytes / nbx_eri_pack / nbx_jk_packed agree on it per process.
 * That kernel uses K = K^T (d_dm symmetric, as the interface asks): its per-slab outputs are symmetrised partials.
 * N = 149 .. 400 run the same walk with a tile in more chunks (csrc/jk_mx.hip: instances at every multiple of eight from
 * 152 to 256, then 272, 288 and every multiple of sixteen from 304 to 400; the same 4 x 4 blocks, stored chunk after
 * chunk -- whole block rows at the top of the triangle, from N = 304 the lower bands of four block rows in segments of
 * column groups; a size between two instances runs as the next one within eight, zero-padded as above;
 * NBX_JK_MX=0 hands N <= 256 back to the layout above and the sizes beyond it to nbx_jk_dense_sym).  These sizes make
 * their Dtot' table themselves (nbx_jk_dts_bytes = 0: nothing to hand over).  Dense + packed tensor must both be
 * resident while nbx_eri_pack runs, which ends at N = 400 on one 288 GB device.
 * N = 97 .. 148 (round 4; csrc/jk_m8.hip, an instance per multiple of four as for jk_m4.hip, unless NBX_JK_M8=0) are stored
 * and contracted 8-FOLD packed -- of tile (p, q) only the elements (rs) <= (pq), the element (rs) = (pq) halved: every
 * integral is in HBM once, 0.63 of the 4-fold form's bytes with the tiles cut at chunk boundaries -- with the same blocks and
 * the same walk; K = Kp + Kp^T, the J term of the mirrored
 * copy as an AXPY in the loading waves' registers (csrc/jk_m8.hip).  nbx_jk_packed_fold says which form a size has.
 *   nbx_jk_packed_fold      : 8 = the packed tensor of this size holds the 8-fold unique integrals, 4 = the 4-fold ones
 *            (q <= p, s <= r), 0 = no packed form
 *   nbx_jk_packed_supported : 1 = a kernel instance serves N (even N <= 256 with N % NB == 0; the sizes above);
 *            2 = N is served as the next such size (at most 8 more) with the extra rows and
 *            columns zero -- odd N, N = 102, 150, 300, ...: the same entry points, the padding is internal
 *            (tiles with p >= N are neither stored nor visited, D is padded on the way in, J/K cropped
 *            on the way out); 0 = not covered (use nbx_jk_dense_sym)
 *   d_jk   : out, ((1+ndm), N, N): ADDITIVE over slabs exactly as nbx_jk_dense_sym
 *   d_work : nbx_jk_packed_worksize() bytes                                                  */
int nbx_jk_packed_supported(int64_t nao);
int nbx_jk_packed_fold(int64_t nao);
size_t nbx_eri_packed_bytes(int64_t nao, int64_t p0, int64_t p1);
int nbx_eri_pack(nbx_ctx* ctx, int64_t nao, int64_t p0, int64_t p1, const double* d_eri, double* d_packed);
size_t nbx_jk_packed_worksize(int64_t nao, int64_t p0, int64_t p1, int64_t ndm);
int nbx_jk_packed(nbx_ctx* ctx, int64_t nao, int64_t p0, int64_t p1, const double* d_packed,
                  const double* d_dm, int64_t ndm, double* d_jk, void* d_work, size_t work_bytes);

/* Test support: which file's kernel nbx_eri_pack / nbx_jk_packed serve a size with IN THIS PROCESS (the switches
 * NBX_JK_M8 / NBX_JK_M4 / NBX_JK_MX are read once per process) and the instance size it runs as (nao itself, or the
 * next instance with zero rows and columns; 0 with NBX_JK_KERNEL_NONE) -- the answer of the one resolver
 * (csrc/jk_packed.hip, packed_resolve) that honours the switches and that every entry point above asks, host
 * arithmetic only (no context, no GPU).  tests/jk_cases.py keeps a size per instance and tests/test_host_jk_cases.py
 * fails when a size of the table moves to another kernel.                                                        */
#define NBX_JK_KERNEL_NONE 0   /* not covered: nbx_jk_dense_sym */
#define NBX_JK_KERNEL_S4 1     /* csrc/jk_s4.hip: the 4-fold tiles walked on the vector ALU */
#define NBX_JK_KERNEL_M4 2     /* csrc/jk_m4.hip: 4-fold 4 x 4 blocks on the matrix cores (NBX_JK_M8=0) */
#define NBX_JK_KERNEL_M8 3     /* csrc/jk_m8.hip: the 8-fold form, N = 97 .. 148 */
#define NBX_JK_KERNEL_MX 4     /* csrc/jk_mx.hip: N = 149 .. 256 */
#define NBX_JK_KERNEL_MX_HI 5  /* csrc/jk_mx_hi.hip: N = 257 .. 400 */
int nbx_jk_packed_route(int64_t nao, int* kernel, int* run_as);

/* nbx_jk_packed over the whole tensor (p0 = 0, p1 = N, two spin densities) with the Fock
 * assembly of nbx_fock_uhf done by its reduction kernel (one launch less per SCF cycle):
 *   d_hv : (2,N,N) hcore + V_emb;  d_fock[x] = d_hv[x] + J - K[x];  d_vhf[x] = J - K[x] (may be
 *   NULL);  d_jk as nbx_jk_packed.  nbed/scf/huzinaga_scf.py:156-160.
 *   d_dts : NULL, or the Dtot' table of d_dm that nbx_huz_cycle_scalars_dts left behind when it
 *   judged this density (saves the build its preparation launch): nbx_jk_dts_bytes() bytes, zeroed
 *   ONCE with nbx_jk_dts_init (the entries it never writes are zero weights).               */
size_t nbx_jk_dts_bytes(int64_t nao);
int nbx_jk_dts_init(nbx_ctx* ctx, int64_t nao, double* d_dts);
int nbx_jk_packed_fock(nbx_ctx* ctx, int64_t nao, const double* d_packed, const double* d_dm,
                       const double* d_hv, double* d_jk, double* d_fock, double* d_vhf, void* d_work,
                       size_t work_bytes, const double* d_dts);

/* Same contraction with the synthetic (pq|rs) of nbx_synth_eri GENERATED in registers instead of
 * read from HBM (the N_AO = 2000 configuration: a dense tensor would be 128 TB).  Workspace as
 * nbx_jk_dense_worksize().  ALU-bound (one 64-bit counter hash per integral).               */
int nbx_jk_synth(nbx_ctx* ctx, int64_t nao, int64_t p0, int64_t p1, uint64_t seed, const double* d_dm,
                 int64_t ndm, double* d_jk, void* d_work, size_t work_bytes);

/* nbx_jk_synth in the additive, symmetric form of nbx_jk_dense_sym: only the tiles q <= p are
 * generated (half the hash evaluations; the kernel is VALU bound).  Even N <= 2048.  d_jk: out,
 * ((1+ndm), N, N) full-size contributions of slab rows [p0,p1), summed across slabs by the host. */
size_t nbx_jk_synth_sym_worksize(int64_t nao, int64_t p0, int64_t p1, int64_t ndm);
int nbx_jk_synth_sym(nbx_ctx* ctx, int64_t nao, int64_t p0, int64_t p1, uint64_t seed,
                     const double* d_dm, int64_t ndm, double* d_jk, void* d_work, size_t work_bytes);

/* ------------------------------------------------------------------ dense products (MFMA fp64)
 * C[b] = alpha * op(A[b]) * op(B[b]) + beta * C[b], row-major, op = 'N' or 'T'.
 * Replaces the OpenBLAS dgemm behind numpy matmul/einsum at
 * nbed/scf/huzinaga_scf.py:78-86,132-134,144-146,166-169; nbed/driver.py:439,446;
 * nbed/localizers/system.py:34-36; nbed/ham_builder.py:76-79;
 * nbed/localizers/occupied/spade.py:98-99,132-134;
 * nbed/localizers/virtual/concentric.py:146-153,175-176,205-207,228,235.      */
int nbx_gemm(nbx_ctx* ctx, char trans_a, char trans_b, int64_t m, int64_t n, int64_t k,
             double alpha, const double* d_a, int64_t lda, int64_t stride_a,
             const double* d_b, int64_t ldb, int64_t stride_b, double beta,
             double* d_c, int64_t ldc, int64_t stride_c, int64_t batch);
/* Test support: which kernel nbx_gemm runs a product on -- the function its launcher calls, host arithmetic only
 * (no context, no GPU; NBX_GEMM_DMA in the environment is honoured as the launcher honours it).  vec_a / vec_b:
 * 1 = the operand has a 16-byte aligned base and even ld and batch stride (what nbx_gemm derives from its
 * arguments), 0 = it is staged element by element.  A batch past 65535 runs in chunks: the answer is for the first.
 * tests/gemm_cases.py keeps a shape per kernel and layout and tests/test_host_gemm_cases.py fails when a retuned
 * threshold moves one of them to another kernel.                                                              */
#define NBX_GEMM_KERNEL_NONE 0   /* nothing launched (m, n or batch == 0) */
#define NBX_GEMM_KERNEL_SMALL 1  /* gemm_small_kernel: one wave per 16 x 16 tile, operands straight from memory */
#define NBX_GEMM_KERNEL_T32 2    /* gemm_f64_kernel, 32 x 32 tiles */
#define NBX_GEMM_KERNEL_T64 3    /* gemm_f64_kernel, 64 x 64 tiles */
#define NBX_GEMM_KERNEL_T128 4   /* gemm_f64_kernel, 128 x 128 tiles */
#define NBX_GEMM_KERNEL_TN_DMA 5 /* gemm_m4_tn_kernel: 'T','N' only, k-tiles brought into LDS by the load unit */
int nbx_gemm_route(char trans_a, char trans_b, int64_t m, int64_t n, int64_t k, int64_t batch, int vec_a,
                   int vec_b);

/* ------------------------------------------------------------------ Fock assembly & reductions */
/* F[x] = hcore[x or 0] + vemb[x] + J - K[x]  (x < 2); d_jk as written by nbx_jk_dense with
 * p0=0,p1=N,ndm=2.  hcore_ndim = 2 -> (N,N) shared, 3 -> (2,N,N).  d_vemb may be NULL.
 * nbed/scf/huzinaga_scf.py:157 (get_veff: vhf = J_a + J_b - K_x).                          */
int nbx_fock_uhf(nbx_ctx* ctx, int64_t nao, const double* d_hcore, int hcore_ndim,
                 const double* d_vemb, const double* d_jk, double* d_fock, double* d_vhf);
/* Huzinaga operator, occupied part (nbed/scf/huzinaga_scf.py:78-80):
 * given FDS[b] = F[b] @ (D_env[b] @ S):  Hz[b] = -kappa (FDS[b] + FDS[b]^T); if d_fock_io
 * is not NULL also F[b] += Hz[b] (:160).                                                    */
int nbx_huzinaga_sym(nbx_ctx* ctx, int64_t nao, int64_t batch, const double* d_fds, double kappa,
                     double* d_hz, double* d_fock_io);
/* out[b] = sum_ij A[b,i,j] * B[b,j,i]   (einsum "ij,ji->"; huzinaga_scf.py:185,
 * embedded_hcore_funcs.py:38-42, driver.py:957-962).  h_out: host, synchronises.          */
/* The same operator from F and DS = D_env S directly, product and symmetrisation in one launch
 * (huzinaga_scf.py:78-81 as one kernel): d_hz[b] = -kappa (F[b] DS[b] + (F[b] DS[b])^T) and, if
 * d_fock_out is not NULL, d_fock_out[b] = F[b] + d_hz[b] (out of place: must not alias d_f).  */
int nbx_huzinaga_fused(nbx_ctx* ctx, int64_t nao, int64_t batch, const double* d_f, const double* d_ds, double kappa,
                       double* d_hz, double* d_fock_out);
int nbx_trace_prod(nbx_ctx* ctx, int64_t nao, int64_t batch, const double* d_a, const double* d_b,
                   double* h_out);
/* Per-cycle scalars of the Huzinaga HF branch (huzinaga_scf.py:181-194):
 *   h_out[x]   = tr[(hcore + vemb[x] + 0.5 vhf[x] + hz[x]) D[x]]      x = 0,1
 *   h_out[2+x] = || D[x] - Dold[x] ||_F                                                     */
int nbx_huz_cycle_scalars(nbx_ctx* ctx, int64_t nao, const double* d_hcore, int hcore_ndim,
                          const double* d_vemb, const double* d_vhf, const double* d_hz,
                          const double* d_dm, const double* d_dm_old, double* h_out);
/* Same scalars (square roots applied) with no synchronisation, so that the host can queue the
 * next SCF cycle before it reads them.  One launch: the workgroup that arrives last does the
 * second stage.  d_out: 4 + tail_n + 1 doubles of device memory or pinned (device-mapped) host
 * memory -- stored to host memory directly the values need no copy.  The LAST word,
 * d_out[4 + tail_n], receives 1.0 after everything before it is visible system-wide: a host that
 * cleared it before the call can poll it instead of recording an event on the stream (an event
 * between two cycles holds the next cycle's first kernel back by ~10 us on MI355X).
 * d_tail (optional): tail_n <= 64 device ints appended as doubles, e.g. the eigensolver status
 * words, so that they reach the host together.                                                */
int nbx_huz_cycle_scalars_dev(nbx_ctx* ctx, int64_t nao, const double* d_hcore, int hcore_ndim,
                              const double* d_vemb, const double* d_vhf, const double* d_hz,
                              const double* d_dm, const double* d_dm_old, double* d_out,
                              const int* d_tail, int64_t tail_n);
/* nbx_huz_cycle_scalars_dev that also prepares the NEXT J/K build: with d_dts (see
 * nbx_jk_packed_fock) the kernel, which reads D anyway, leaves Dtot' of d_dm in the table.     */
int nbx_huz_cycle_scalars_dts(nbx_ctx* ctx, int64_t nao, const double* d_hcore, int hcore_ndim,
                              const double* d_vemb, const double* d_vhf, const double* d_hz,
                              const double* d_dm, const double* d_dm_old, double* d_out, const int* d_tail,
                              int64_t tail_n, double* d_dts);
/* One pyscf.lib.diis.DIIS.update step (behind huzinaga_scf.py:130,164) with nothing leaving
 * the device.  State: d_xs, d_es = (space, n) trial / error vectors, d_h = the
 * (space+1)x(space+1) Pulay matrix (row 0 / column 0 = 1, H[0][0] = 0; the caller initialises
 * it once), d_xprev = the vector returned by the previous update.  The call stores x in slot
 * `slot`, e = x - xprev beside it, fills row/column slot+1 of H with <e_slot|e_k> (k < nd, nd
 * counts the vectors held including this one), solves H[:nd+1,:nd+1] c = (1,0,...) with
 * PySCF's rule (modes with |eigenvalue| < 1e-14 are dropped when there are any, otherwise an
 * LU solve), and overwrites d_xprev with sum_k c[k+1] xs[k]: the extrapolated vector.
 * d_coef: nbx_diis_coef_doubles(space) doubles, ZERO-INITIALISED by the caller before the first
 * update of a ring and left alone afterwards: c[1:] in the first `space` of them, behind them
 * the solver's own state (the eigenvector basis its Jacobi sweeps ended in, from which the next
 * update's solve starts: one row / column of H changes per update).  1 <= nd <= space <= 16.   */
size_t nbx_diis_coef_doubles(int64_t space);
int nbx_diis_update(nbx_ctx* ctx, int64_t n, int64_t space, int64_t slot, int64_t nd,
                    const double* d_x, double* d_xprev, double* d_xs, double* d_es, double* d_h,
                    double* d_coef);
/* The same step with the error vector supplied by the caller (d_err, n doubles) instead of
 * x - xprev: pyscf.scf.diis.CDIIS (error S D F - F D S, space 8) behind scf.hf.kernel, which the
 * mu-shift path runs (nbed/driver.py:533).  d_xprev only receives the extrapolated vector.     */
int nbx_diis_update_err(nbx_ctx* ctx, int64_t n, int64_t space, int64_t slot, int64_t nd,
                        const double* d_x, const double* d_err, double* d_xprev, double* d_xs,
                        double* d_es, double* d_h, double* d_coef);
/* d_out[x] = sum_{a >= nocc_x, i < nocc_x} fmo[x][a][i]^2 for the (2,N,N) MO-basis Fock matrix
 * C^T F C: the squared norm of the orbital gradient PySCF's scf.hf.kernel tests for convergence
 * (get_grad + norm/sqrt(size), behind nbed/driver.py:533).  Device output, no synchronisation.  */
int nbx_vo_sumsq(nbx_ctx* ctx, int64_t nao, const double* d_fmo, int64_t nocc_a, int64_t nocc_b,
                 double* d_out);
/* y = a*x + b*y over n doubles. */
int nbx_axpby(nbx_ctx* ctx, int64_t n, double a, const double* d_x, double b, double* d_y);
/* out = sum_k coef[k] * vecs[k] (k < nvec; vecs[k] = d_vecs + k*stride), DIIS extrapolation
 * (pyscf.lib.diis.DIIS.extrapolate behind huzinaga_scf.py:164).                             */
int nbx_lincomb(nbx_ctx* ctx, int64_t n, int64_t nvec, const double* h_coef, const double* d_vecs,
                int64_t stride, double* d_out);
/* h_out[k] = <x, vecs[k]>, k < nvec (DIIS B-matrix row). Synchronises. */
int nbx_dots(nbx_ctx* ctx, int64_t n, int64_t nvec, const double* d_x, const double* d_vecs,
             int64_t stride, double* h_out);
/* B[b] = A[b]^T for (rows x cols) matrices. */
int nbx_transpose(nbx_ctx* ctx, int64_t rows, int64_t cols, int64_t batch, const double* d_a,
                  double* d_b);
/* A[:, j] *= s[j]  (columns scaled; row-major (rows x cols)). */
int nbx_scale_cols(nbx_ctx* ctx, int64_t rows, int64_t cols, int64_t batch, const double* d_s,
                   double* d_a);
/* Test support, like nbx_gemm_route: which kernel instance the launch functions above pick -- the functions they
 * call themselves, host arithmetic only (no context, no GPU), and the only statement of these limits.
 * tests/scf_kernel_cases.py keeps shapes per instance and tests/test_host_scf_kernel_cases.py fails when a retuned
 * threshold moves one of them.
 * nbx_cycle_scalars_route: the energy / |dD| scalars of a cycle.  nocc_a = nocc_b = -1: of given matrices
 * (nbx_huz_cycle_scalars_dev / _dts and the mu-shift cycle: 16 x 16 tiles while their partial sums fit the context's
 * scratch, 32 x 32 tiles while those fit, refused beyond).  nocc_a, nocc_b >= 0: inside nbx_huz_cycle -- T16_DENS
 * where the kernel also makes the aufbau density (16 x 16 tiles, both spins occupied and no wider than the kernel's
 * operand registers), else what the density product + the form above run on.  The limits themselves are stated in
 * csrc/elementwise.hip (scalars_route, density_scalars_fused) and nowhere else: ask this function.
 * (The synchronous nbx_huz_cycle_scalars always runs on 32 x 32 tiles and is refused where T32 would be.)          */
#define NBX_CYCLE_SCALARS_REFUSED 0
#define NBX_CYCLE_SCALARS_T32 1      /* huz_scalars_kernel<32> */
#define NBX_CYCLE_SCALARS_T16 2      /* huz_scalars_kernel<16> */
#define NBX_CYCLE_SCALARS_T16_DENS 3 /* huz_scalars_kernel<16, true>: density and scalars in one launch */
int nbx_cycle_scalars_route(int64_t nao, int64_t nocc_a, int64_t nocc_b);
/* nbx_diis_update / _err on vectors of n doubles with nd vectors held: the Pulay solve and the extrapolation in one
 * kernel while the Pulay matrix fits one element per lane, or the general solver followed by the linear combination
 * (diis_route in csrc/elementwise.hip).                                                                          */
#define NBX_DIIS_REFUSED 0
#define NBX_DIIS_FUSED 1   /* diis_solve8_lincomb_kernel */
#define NBX_DIIS_GENERAL 2 /* diis_solve_kernel + lincomb_dev_kernel */
int nbx_diis_route(int64_t n, int64_t nd);
/* nbx_vo_sumsq: one workgroup per spin that stores its sum (small virtual-occupied blocks), or 32 per spin and a
 * second stage (vo_sumsq_route in csrc/elementwise.hip).                                                          */
#define NBX_VO_SUMSQ_REFUSED 0
#define NBX_VO_SUMSQ_ONE_WG 1
#define NBX_VO_SUMSQ_32_WG 2
int nbx_vo_sumsq_route(int64_t nao, int64_t nocc_a, int64_t nocc_b);

/* ------------------------------------------------------------------ symmetric eigensolver
 * Replaces np.linalg.eigh (LAPACK dsyevd) at nbed/scf/huzinaga_scf.py:145,168 and the
 * eigensolve inside fractional_matrix_power at :128 / spade.py:99.
 * d_a: (batch,N,N) symmetric, preserved.  d_w: (batch,N) ascending.  d_v: (batch,N,N),
 * columns = eigenvectors.  Cyclic two-sided Jacobi (parallel ordering) for N < 64; Householder reduction,
 * Sturm multisection, inverse iteration and back-transformation above (csrc/eigh_tridiag.hip: the matrix in one
 * workgroup's registers up to N = 198; csrc/eigh_grid.hip beyond: the matrix in the LDS of up to 256 workgroups,
 * one grid-wide hand-over per Householder step -- a COOPERATIVE launch, so the call needs the device's CUs to itself
 * for its duration -- and the back-transformation in compact-WY blocks on the GEMM; N <= 2048), Jacobi as the
 * polisher when a cluster defeats inverse iteration.
 * d_work: nbx_eigh_worksize() bytes.  Returns NBX_E_NOCONV if max sweeps hit.             */
size_t nbx_eigh_worksize(int64_t n, int64_t batch);
int nbx_eigh(nbx_ctx* ctx, int64_t n, int64_t batch, const double* d_a, double* d_w, double* d_v,
             void* d_work, size_t work_bytes);
/* Warm start: d_v0 (batch,N,N) holds approximate eigenvectors (orthonormal columns, e.g. the
 * previous SCF cycle's).  For N <= 196 the pair is first refined with GEMMs only (Ogita-Aishima
 * iteration, 3 steps, quadratically convergent); a matrix the refinement does not bring to
 * max|E| < 3e-8 -- or that has coupled near-degenerate eigenvalues -- falls through, on the
 * device and with no host round trip, to Jacobi sweeps on V0^T A V0 (nearly diagonal: 1-4
 * sweeps instead of 8-10).  d_v0 == NULL is nbx_eigh.  Same outputs/workspace.               */
int nbx_eigh_warm(nbx_ctx* ctx, int64_t n, int64_t batch, const double* d_a, const double* d_v0,
                  double* d_w, double* d_v, void* d_work, size_t work_bytes);
/* Same with the number of refinement iterations queued before the Jacobi fallback chosen by the
 * caller (0 = none, 3 = the default of nbx_eigh_warm, 6 = most).  Results do not depend on it -- a matrix the queued
 * iterations do not finish is solved by the sweeps -- only the number of launches does: an SCF
 * driver that saw the last cycles accepted after one iteration queues one.                   */
int nbx_eigh_warm_ex(nbx_ctx* ctx, int64_t n, int64_t batch, const double* d_a, const double* d_v0,
                     double* d_w, double* d_v, void* d_work, size_t work_bytes, int refine_iters);
/* Byte offset inside the nbx_eigh workspace of the int[batch] status words nbx_eigh_status reads,
 * for callers that fetch them with their own stream-ordered copy instead of synchronising.   */
size_t nbx_eigh_status_offset(int64_t n, int64_t batch);
/* Reads back the sweep counts of the last nbx_eigh on this workspace (synchronises):
 * h_sweeps[b] > 0 = sweeps used (1000 + k: accepted by the warm-start refinement after k
 * iterations, no sweeps); returns NBX_E_NOCONV if any matrix hit the sweep limit.          */
int nbx_eigh_status(nbx_ctx* ctx, int64_t n, int64_t batch, const void* d_work, int* h_sweeps);
/* Eigenpairs to inverse-iteration accuracy with nothing read back: Householder reduction, multisection,
 * inverse iteration, back-transformation and one Newton-Schulz orthonormalisation step, all queued (the cold
 * route of nbx_eigh without its two host decisions).  A START for nbx_eigh_warm_ex / nbx_huz_cycle mode 0 on
 * the same or a nearby matrix -- e.g. solved on a second stream beside SCF cycles that do not need orbitals
 * (nbx_huz_cycle mode 2) -- not a result: d_status[b] = 1 the vectors are orthonormal to ~1e-12 (their
 * residual is whatever inverse iteration left, typically 1e-10 ||A||); -1 clustered levels left nearly
 * dependent vectors (or NaN): do not use them.  n <= 2048.                                          */
size_t nbx_eigh_approx_worksize(int64_t n, int64_t batch);
int nbx_eigh_approx(nbx_ctx* ctx, int64_t n, int64_t batch, const double* d_a, double* d_w, double* d_v,
                    void* d_work, size_t work_bytes, int* d_status);
/* out = S^p for symmetric positive definite S (N,N): U diag(w^p) U^T.
 * scipy.linalg.fractional_matrix_power(S, -0.5 / +0.5) at nbed/scf/huzinaga_scf.py:128,
 * nbed/localizers/occupied/spade.py:99; np.linalg.inv(S_AA) at
 * nbed/localizers/virtual/concentric.py:147 (p = -1).                                      */
size_t nbx_sym_pow_worksize(int64_t n);
/* The same power, p in {-1/2, +1/2, -1}, of a symmetric POSITIVE DEFINITE S by the coupled Newton-Schulz iteration
 * (three GEMMs per step, ~0.2 ms at N = 148 where the eigen route takes ~1-3 ms): c = a bound of the spectrum (the
 * caller's ||S||_inf), convergence (||I - Z Y||_F) read back every `check_every` steps.  *h_iters = steps taken, or -1
 * when it did not converge within max_iter (not positive definite, condition number beyond ~1e6): d_out is then
 * untouched and the caller takes nbx_sym_pow.  Agrees with fractional_matrix_power to ~cond(S) 1e-16.  Synchronises. */
size_t nbx_sym_pow_ns_worksize(int64_t n);
int nbx_sym_pow_ns(nbx_ctx* ctx, int64_t n, const double* d_s, double p, double c, double* d_out, void* d_work,
                   size_t work_bytes, int max_iter, int check_every, int* h_iters);
int nbx_sym_pow(nbx_ctx* ctx, int64_t n, const double* d_s, double p, double* d_out,
                void* d_work, size_t work_bytes);

/* ------------------------------------------------------------------ SVD (right vectors)
 * Replaces scipy.linalg.svd / np.linalg.svd (LAPACK dgesdd) at
 * nbed/localizers/occupied/spade.py:101 and nbed/localizers/virtual/concentric.py:151,205: A (m x n) -> s (min(m,n)) descending, Vt (n x n) with rows the
 * right singular vectors (full_matrices=True semantics).  One-sided Jacobi.              */
size_t nbx_svd_worksize(int64_t m, int64_t n);
int nbx_svd_right(nbx_ctx* ctx, int64_t m, int64_t n, const double* d_a, double* d_s, double* d_vt,
                  void* d_work, size_t work_bytes);
/* Generalised symmetric eigenproblem F C = S C eps by iterative refinement of the PREVIOUS SCF
 * cycle's solution (Ogita-Aishima on the pencil: G = C^T S C, S~ = C^T F C, C <- C (I + E)), all
 * GEMMs -- what scipy.linalg.eigh(F, S) / the Loewdin route of nbed/scf/huzinaga_scf.py:166-169
 * computes, once an SCF is under way.  batch matrices: d_f, d_s (the overlap, repeated per batch
 * entry), d_c0 (S-orthonormal start vectors), all (batch, n, n) row-major.
 *   d_status[b] = 1000 + iterations used: accepted, d_w[b] (ascending) and d_c[b] written;
 *               <= 0: not converged within max_iter (1..6), near-degenerate cluster coupled, or
 *                     (max_iter = 1, where no sorting pass is queued) the eigenvalue order has
 *                     changed -- outputs not valid.  There is NO fallback solver behind this entry: the
 *                     caller checks the status (the SCF loops do, one cycle late, and redo the run
 *                     on nbx_eigh_warm_ex if it ever fails).
 * Nothing synchronises.  d_work: nbx_geig_refine_worksize() bytes.                              */
size_t nbx_geig_refine_worksize(int64_t n, int64_t batch);
int nbx_geig_refine(nbx_ctx* ctx, int64_t n, int64_t batch, const double* d_f, const double* d_s,
                    const double* d_c0, double* d_w, double* d_c, int* d_status, void* d_work,
                    size_t work_bytes, int max_iter);

/* nbx_ao2mo_pair for C1 = C2 (one matrix d_c12, n columns) over the whole outer range:
 * (ij|kl) = (ji|kl), so quarters 3 and 4 run on the pairs j <= i only and each finished (k,l)
 * block is stored at (i,j) and (j,i).  Every ao2mo.kernel call of nbed/ham_builder.py:127-133
 * has C1 = C2.  Same outputs as nbx_ao2mo_pair up to rounding ((i,j) and (j,i) are equal by
 * construction here); d_out2 == NULL: one tensor.  Outer-index slabs, or n > 361 (more than 65535
 * pairs: NBX_E_UNSUPPORTED): use nbx_ao2mo_pair.                                               */
size_t nbx_ao2mo_pair_sym_worksize(int64_t nao, int64_t n, int64_t n4, int64_t n6);
/* ... and with (pq|rs) = (pq|sr) too: nbx_eri_pack_rs stores (r, s <= r) packed once per molecule
 * (out[(p,q)][r(r+1)/2 + s], nbx_eri_rs_bytes() bytes -- PySCF's "s2kl" form of ao2mo's input);
 * quarters 1 and 2 of nbx_ao2mo_pair_sym_rs then run on N(N+1)/2 columns instead of N^2 and
 * quarter 3 reads the packed X2 in place.  Same results as nbx_ao2mo_pair_sym up to rounding.  */
size_t nbx_eri_rs_bytes(int64_t nao);
int nbx_eri_pack_rs(nbx_ctx* ctx, int64_t nao, const double* d_eri, double* d_out);
size_t nbx_ao2mo_pair_sym_rs_worksize(int64_t nao, int64_t n, int64_t n4, int64_t n6);
int nbx_ao2mo_pair_sym_rs(nbx_ctx* ctx, int64_t nao, const double* d_eri_rs, const double* d_c12, int64_t n,
                          const double* d_c3, int64_t n3, const double* d_c4, int64_t n4, double* d_out,
                          const double* d_c5, int64_t n5, const double* d_c6, int64_t n6, double* d_out2,
                          void* d_work, size_t work_bytes);
int nbx_ao2mo_pair_sym(nbx_ctx* ctx, int64_t nao, const double* d_eri, const double* d_c12, int64_t n,
                       const double* d_c3, int64_t n3, const double* d_c4, int64_t n4, double* d_out,
                       const double* d_c5, int64_t n5, const double* d_c6, int64_t n6, double* d_out2,
                       void* d_work, size_t work_bytes);

/* Sweep count of the last nbx_svd_right on this workspace (synchronises); NBX_E_NOCONV if the
 * sweep limit was hit. */
int nbx_svd_status(nbx_ctx* ctx, int64_t m, int64_t n, const void* d_work, int* h_sweeps);

/* ------------------------------------------------------------------ Localisation (Pipek-Mezey, Boys)
 * Replaces pyscf.lo.PipekMezey(mol, C).kernel() and pyscf.lo.boys.Boys(mol, C).kernel() at
 * nbed/localizers/occupied/pyscf.py:317-324,378-379: the orthogonal U (n x n) that maximises
 * f(U) = sum_k sum_i ((U^T Q_k U)_ii)^2 by Jacobi sweeps; C_loc = C U.  One workgroup per problem, every sweep in
 * one launch (csrc/localize.hip).
 *   nbx_loc_pm    Q_A = 1/2 (X_A^T Y_A + Y_A^T X_A) over the AO rows [h_ao_offsets[A], h_ao_offsets[A+1]) of each
 *                 atom; d_x, d_y (batch, nao, n) row-major, d_y NULL: Y = X.  h_ao_offsets: natm + 1 host values
 *                 ascending from 0 to nao.  Copies them to the workspace (synchronises).
 *   nbx_loc_boys  d_q (batch, 3, n, n) symmetric: C^T r_k C, k = x, y, z.
 * d_u (batch, n, n).  The sweeps stop once a whole sweep's largest |sin gamma| is below tol, or after max_sweeps
 * (d_u is written either way).  d_work: nbx_loc_worksize(kind, ...) bytes, kind NBX_LOC_PM or NBX_LOC_BOYS (Boys
 * ignores nao and natm); too small: NBX_E_INVALID.  Identical inputs give bit-identical outputs.
 * nbx_loc_status (synchronises) returns the sweeps and f of each problem of the last call on the workspace, and
 * NBX_E_NOCONV if any problem hit max_sweeps.                                                        */
#define NBX_LOC_PM 0
#define NBX_LOC_BOYS 1
size_t nbx_loc_worksize(int kind, int batch, int64_t nao, int64_t n, int64_t natm);
int nbx_loc_pm(nbx_ctx* ctx, int batch, int64_t nao, int64_t n, int64_t natm, const int64_t* h_ao_offsets,
               const double* d_x, const double* d_y, double* d_u, int max_sweeps, double tol, void* d_work,
               size_t work_bytes);
int nbx_loc_boys(nbx_ctx* ctx, int batch, int64_t n, const double* d_q, double* d_u, int max_sweeps, double tol,
                 void* d_work, size_t work_bytes);
int nbx_loc_status(nbx_ctx* ctx, int batch, const void* d_work, int* h_sweeps, double* h_f);

/* ------------------------------------------------------------------ four-index transform
 * Replaces pyscf.ao2mo.kernel + ao2mo.restore(1, ...) at nbed/ham_builder.py:127-131:
 *   out[i-i0,j,k,l] = sum_pqrs C1[p,i] C2[q,j] C3[r,k] C4[s,l] (pq|rs),  i in [i0,i1)
 * d_eri dense (N,N,N,N); Cx are (N,nx) row-major.  Four quarter transforms (MFMA GEMMs).
 * The outer MO index i is the multi-GPU shard axis.                                       */
size_t nbx_ao2mo_worksize(int64_t nao, int64_t ni, int64_t n2, int64_t n3, int64_t n4);
int nbx_ao2mo(nbx_ctx* ctx, int64_t nao, const double* d_eri, const double* d_c1, int64_t n1,
              int64_t i0, int64_t i1, const double* d_c2, int64_t n2, const double* d_c3,
              int64_t n3, const double* d_c4, int64_t n4, double* d_out, void* d_work,
              size_t work_bytes);
/* Two tensors that share their first two MO indices in one pass,
 *   out [i-i0,j,k,l] = (C1 C2 | C3 C4),   out2[i-i0,j,k,l] = (C1 C2 | C5 C6):
 * quarters 1 and 2 are computed once.  The unrestricted Hamiltonian needs (aa|aa), (bb|bb) and
 * (aa|bb) (nbed/ham_builder.py:127-133, three independent ao2mo.kernel calls in the reference):
 * (aa|aa) and (aa|bb) are such a pair, which removes a third of the quarter-1 work.  Results are
 * bitwise those of two nbx_ao2mo calls.  d_out2 == NULL: plain nbx_ao2mo.                    */
size_t nbx_ao2mo_pair_worksize(int64_t nao, int64_t ni, int64_t n2, int64_t n4, int64_t n6);
int nbx_ao2mo_pair(nbx_ctx* ctx, int64_t nao, const double* d_eri, const double* d_c1, int64_t n1,
                   int64_t i0, int64_t i1, const double* d_c2, int64_t n2, const double* d_c3,
                   int64_t n3, const double* d_c4, int64_t n4, double* d_out, const double* d_c5,
                   int64_t n5, const double* d_c6, int64_t n6, double* d_out2, void* d_work,
                   size_t work_bytes);
/* Streamed transform of the synthetic (pq|rs) of nbx_synth_eri, never stored (N_AO = 2000).
 * (pq|rs) = (pq|sr) is used: only the pairs s <= r are generated and half-transformed (the
 * symmetry PySCF's ao2mo, which the reference calls, uses as well).  The call returns the part
 * of the sum that belongs to r in [r0,r1), i.e. all pairs (r, s <= r) and their mirror images:
 *   out[i,j,k,l] = sum_{r in [r0,r1)} sum_{s<=r} sum_pq C1[p,i] C2[q,j] (pq|rs)
 *                                   (C3[r,k] C4[s,l] + [s<r] C3[s,k] C4[r,l])
 * [r0,r1) is the multi-GPU shard axis: the partial tensors of the ranks are SUMMED (all-reduce)
 * by the host; the work of a range grows with r, so equal-work ranges are not equal-length.   */
size_t nbx_ao2mo_synth_worksize(int64_t nao, int64_t n1, int64_t n2, int64_t n3, int64_t n4);
/* ... and the pair form of it (see nbx_ao2mo_pair): out2 = (C1 C2|C5 C6) beside out, the generated
 * integrals and quarters 1-2 shared.  d_out2 == NULL: nbx_ao2mo_synth.                        */
size_t nbx_ao2mo_synth_pair_worksize(int64_t nao, int64_t n1, int64_t n2, int64_t n3, int64_t n4,
                                     int64_t n5, int64_t n6);
int nbx_ao2mo_synth_pair(nbx_ctx* ctx, int64_t nao, uint64_t seed, int64_t r0, int64_t r1,
                         const double* d_c1, int64_t n1, const double* d_c2, int64_t n2,
                         const double* d_c3, int64_t n3, const double* d_c4, int64_t n4, double* d_out,
                         const double* d_c5, int64_t n5, const double* d_c6, int64_t n6, double* d_out2,
                         void* d_work, size_t work_bytes);
int nbx_ao2mo_synth(nbx_ctx* ctx, int64_t nao, uint64_t seed, int64_t r0, int64_t r1, const double* d_c1,
                    int64_t n1, const double* d_c2, int64_t n2, const double* d_c3, int64_t n3,
                    const double* d_c4, int64_t n4, double* d_out, void* d_work, size_t work_bytes);
/* out[a,c,d,b] = in[a,b,c,d]: chemist (ij|kl) -> the reference's physicist-ordered block
 * eri.transpose(0,2,3,1) (ham_builder.py:133).                                            */
int nbx_chem_to_phys(nbx_ctx* ctx, int64_t n1, int64_t n2, int64_t n3, int64_t n4,
                     const double* d_in, double* d_out);
/* Spin-orbital scatter + truncation (nbed/ham_builder.py:158-216) and the 0.5 factor of
 * build() (:254):  h1 (2n,2n), h2 (2n,2n,2n,2n) from one_body (2,n,n), two_body (4,n,n,n,n);
 * entries with |x| < tol are zeroed; h2 is multiplied by h2_scale afterwards.            */
int nbx_spinorb_scatter(nbx_ctx* ctx, int64_t n, const double* d_one_body, const double* d_two_body,
                        double tol, double h2_scale, double* d_h1, double* d_h2);
/* Elements [idx0, idx0 + count) of the flattened (2n)^4 tensor only, into d_h2_part[0..count): lets
 * a host that wants the result in its own memory stream it out piece by piece instead of holding
 * the whole tensor (60 GB at n = 147) on the device first; nbx_spinorb_scatter_h1 is the one-body
 * part alone (nbed/ham_builder.py:180-214, as nbx_spinorb_scatter).                             */
int nbx_spinorb_scatter_h1(nbx_ctx* ctx, int64_t n, const double* d_one_body, double tol, double* d_h1);
int nbx_spinorb_scatter_range(nbx_ctx* ctx, int64_t n, const double* d_two_body, double tol,
                              double h2_scale, int64_t idx0, int64_t count, double* d_h2_part);

/* ------------------------------------------------------------------ fused SCF cycle
 * One Huzinaga-projected UHF cycle of nbed/scf/huzinaga_scf.py:154-201 queued by ONE call (the chain is
 * 12-40 launches; issued one by one from the host language the first cycles of an SCF are host bound).
 * The caller fills the state once per SCF -- every pointer a device pointer it owns -- and rotates the
 * per-cycle result buffers itself; nothing here allocates or synchronises.  Same kernels, order and
 * operands as the step-by-step entry points: bit-identical results.
 *   mode 1 ("tracked"): nbx_geig_refine from d_c_in = the previous cycle's S-orthonormal C; status in
 *          d_status_out.  mode 0 ("guarded"): X F X, nbx_eigh_warm_ex warm-started from d_c_in = the previous
 *          cycle's orthonormal-basis vectors (NULL: cold), C = X V; d_v_out receives V.
 *          mode 2 ("purified"): no eigenvectors at all -- D = X P X with P the projector on the occupied
 *          levels of X F X from nbx_purify (refine_iters caps its steps, <= 0: the limit); d_c_out and
 *          d_w_out are NOT written, d_v_out (if given) receives X F X -- the matrix an eigensolver would
 *          have been given, so that the cycle's orbitals can be had later or beside the next cycles on
 *          another stream; the status words are nbx_purify's.  For the first cycles of a run, whose
 *          Fock matrix moves too much for a warm-started eigensolver.
 *   diis_mode 0: no DIIS; 1: pyscf.lib.diis' first update (only remembers F); 2: nbx_diis_update with
 *          (diis_slot, diis_nd) -- the ring bookkeeping stays with the caller.
 *   dts_ready: st->d_dts holds the Dtot' table of d_dm_in (left by the previous call).
 *   h_out: 7 doubles of pinned (device-mapped) host memory: E_alpha, E_beta, |dD_alpha|, |dD_beta|, the
 *          eigensolver's two status words, then 1.0 -- stored last, once the six are visible to the host, which
 *          can clear that word before the call and poll it (see nbx_huz_cycle_scalars_dev).          */
typedef struct nbx_huz_state {
    int64_t nao, nocc_a, nocc_b;
    const double* d_packed; /* nbx_eri_pack of the whole tensor / of this rank's slab (NBX_HUZ_JK_PACKED) */
    const double* d_hv;     /* (2,N,N) hcore + V_emb */
    const double* d_ds;     /* (2,N,N) D_env S */
    const double* d_sb;     /* (2,N,N) the overlap, once per spin (tracked mode) */
    const double* d_x;      /* (N,N) S^-1/2 (guarded mode) */
    double* d_dts;          /* nbx_jk_dts_bytes() table or NULL */
    double* d_jk;           /* (3,N,N) */
    double* d_fock;         /* (2,N,N) h + V + vhf */
    double* d_vhf;          /* (2,N,N) */
    double* d_fock2;        /* (2,N,N) ... + Hz */
    double* d_tmp;          /* (2,N,N) guarded mode */
    double* d_fo;           /* (2,N,N) guarded mode */
    void* d_jk_work;
    size_t jk_work_bytes;   /* nbx_jk_packed_worksize / nbx_jk_dense_sym_worksize (nao, p0, p1, 2) */
    void* d_eig_work;
    size_t eig_work_bytes;  /* nbx_eigh_worksize(nao, 2) */
    void* d_geig_work;
    size_t geig_work_bytes; /* nbx_geig_refine_worksize(nao, 2) */
    int64_t diis_space;
    double* d_diis_xs;      /* (space, 2 N^2) */
    double* d_diis_es;
    double* d_diis_h;       /* (space+1)^2, initialised by the caller (row/column 0 = 1) */
                            /* d_diis_coef: nbx_diis_coef_doubles(space) doubles, zeroed by the caller */
    double* d_diis_coef;
    double* d_diis_xprev;   /* 2 N^2 */
    /* which J/K kernel builds the Fock matrix, and on which rows of (pq|rs) */
    int64_t jk_kind;        /* NBX_HUZ_JK_PACKED: d_packed (nbx_jk_packed[_fock]); NBX_HUZ_JK_SYM: d_eri, the dense
                               tensor / row slab (nbx_jk_dense_sym: every N, falls to nbx_jk_dense inside) */
    int64_t jk_p0, jk_p1;   /* this rank's slab rows [p0, p1) of the first AO index: 0, nao = the whole tensor;
                               p0 == p1 = an empty slab (contributes zero) */
    const double* d_eri;    /* NBX_HUZ_JK_SYM: slab rows [p0, p1) of the dense (N,N,N,N) tensor */
    double* d_scal_partial; /* NBX_HUZ_PARTIAL_DOUBLES doubles, 16-byte aligned, or NULL: the partial sums of a cycle
                               whose scalars are deferred (nbx_huz_cycle_carry); nothing else writes them */
} nbx_huz_state;
#define NBX_HUZ_JK_PACKED 0
#define NBX_HUZ_JK_SYM 1
#define NBX_HUZ_PARTIAL_DOUBLES 4096
int nbx_huz_cycle(nbx_ctx* ctx, const nbx_huz_state* st, const double* d_dm_in, const double* d_c_in,
                  double* d_dm_out, double* d_c_out, double* d_v_out, double* d_w_out, double* d_hz_out, int mode,
                  int refine_iters, int diis_mode, int diis_slot, int diis_nd, int dts_ready, double* h_out,
                  int* d_status_out);
/* The same cycle in two calls for runs over several GPUs (one process per GPU): the J/K
 * contribution of this rank's slab of (pq|rs) rows into st->d_jk ((3,N,N), additive over slabs) --
 *     nbx_huz_cycle_jk;   all-reduce (sum) of st->d_jk queued on the same stream by the caller (RCCL);
 *     nbx_huz_cycle_post: Fock assembly from the summed J/K (nbx_fock_uhf) and the rest of the cycle exactly
 * as nbx_huz_cycle queues it -- so every rank keeps the one-cycle look-ahead, the purified early cycles and the
 * tracked eigensolver, and (the replicated part being deterministic) holds bitwise the same matrices.
 * nbx_huz_cycle itself takes this route, without the collective, whenever the state is not "packed kernel on the
 * whole tensor" (N < 100, sizes without a packed instance: NBX_HUZ_JK_SYM).  st->d_dts is not used by _jk. */
int nbx_huz_cycle_jk(nbx_ctx* ctx, const nbx_huz_state* st, const double* d_dm_in);
int nbx_huz_cycle_post(nbx_ctx* ctx, const nbx_huz_state* st, const double* d_dm_in, const double* d_c_in,
                       double* d_dm_out, double* d_c_out, double* d_v_out, double* d_w_out, double* d_hz_out, int mode,
                       int refine_iters, int diis_mode, int diis_slot, int diis_nd, double* h_out, int* d_status_out);
/* Deferred scalars.  The last stage of the kernel that stores a cycle's seven doubles to the host (the sums over the
 * workgroups' partials, the host stores) is on the path to the next cycle's J/K build, which needs only the density
 * and the Dtot' table from that kernel.  A cycle queued with defer != 0 stops at the partial sums (st->d_scal_partial) and describes what
 * is left to do in *deferred_out; the caller hands that description to the NEXT nbx_huz_cycle_carry call as `carry`,
 * whose J/K build takes the scalars to h_out of the deferred cycle in its first trip to memory (one wavefront; the same
 * sums in the same order: bit-identical values, the ready word last), or to nbx_huz_scalars_flush when no cycle follows.
 *   carry:        NULL or d_partial == NULL: nothing to carry -- no host slot but this cycle's own h_out is written.
 *                 Where this call's build cannot carry (not the 8-fold packed kernel on the whole tensor) the scalars
 *                 are flushed by a launch of their own ahead of the build.
 *   defer:        a request.  Granted only where the next build could carry (the 8-fold packed kernel on the whole
 *                 tensor, st->d_scal_partial given, a scalars launch the courier is written for); otherwise the cycle
 *                 stores its scalars itself as nbx_huz_cycle does and deferred_out->d_partial is NULL.
 *   deferred_out: required when defer != 0.  Nothing is remembered between calls: what is carried is what the caller
 *                 states.  A deferred cycle's h_out receives nothing until a later call carries or flushes it, so a
 *                 host that polls its ready word must have queued that call first.
 * nbx_huz_cycle(..) is nbx_huz_cycle_carry(.., NULL, 0, NULL).                                                      */
typedef struct nbx_scalars_courier {
    const double* d_partial; /* nblocks x 4 partial sums of the scalars kernel (device, 16-byte aligned) */
    int32_t nblocks;         /* workgroups of that launch */
    int32_t nthreads;        /* threads per workgroup of that launch: 128 or 256 */
    const int32_t* d_status; /* the status words that travel with the scalars (device) */
    int32_t nstatus;
    int32_t reserved;
    double* h_out;           /* pinned (device-mapped) host memory: 4 + nstatus + 1 doubles */
} nbx_scalars_courier;
int nbx_huz_cycle_carry(nbx_ctx* ctx, const nbx_huz_state* st, const double* d_dm_in, const double* d_c_in,
                        double* d_dm_out, double* d_c_out, double* d_v_out, double* d_w_out, double* d_hz_out, int mode,
                        int refine_iters, int diis_mode, int diis_slot, int diis_nd, int dts_ready, double* h_out,
                        int* d_status_out, const nbx_scalars_courier* carry, int defer,
                        nbx_scalars_courier* deferred_out);
/* The final stage of a deferred cycle as a launch of its own (one wavefront), queued on the context's stream. */
int nbx_huz_scalars_flush(nbx_ctx* ctx, const nbx_scalars_courier* carry);

/* ------------------------------------------------------------------ fused mu-shift SCF cycle
 * One cycle of the SCF the mu-shift embedding runs -- `embedded_scf.kernel()` at nbed/driver.py:533 on the hcore
 * patched with mu S D_env S + V_emb (:500-538), i.e. PySCF's scf.hf.kernel: CDIIS from cycle 1, eig, aufbau
 * density, get_veff, energy_tot, |dE| and orbital-gradient test -- queued by ONE call, nothing synchronises.
 * Also the global mean field's kernel() (driver.py:112-191).  The state block is nbx_huz_state with
 *   d_hv        = the kernel's h1e per spin (2,N,N)  (hcore + mu P + V_emb, or hcore twice);
 *   d_sb, d_x, d_jk, d_tmp, d_fo, d_fock2 (scratch), the J/K, eigensolver and refinement workspaces as for
 *   nbx_huz_cycle; d_ds, d_fock, d_vhf, d_dts unused (may be NULL);
 *   the DIIS ring for CDIIS: diis_space = 8, d_diis_xs / d_diis_es (8, 2 N^2), d_diis_h (9 x 9, row/column 0 = 1),
 *   d_diis_coef zeroed, d_diis_xprev (2 N^2) receives the extrapolated Fock matrix.
 * Cycle:  [diis_on: err = F D S - S D F of (d_dm_in, d_fock_in) per spin, pyscf.lib.diis.DIIS.update(F, err) with the
 *   caller's ring position (diis_slot, diis_nd)]  ->  F C = S C eps (mode 0 guarded: Loewdin step + nbx_eigh_warm_ex
 *   warm-started from d_c_in = the previous cycle's d_v_out, NULL = cold; mode 1 tracked: nbx_geig_refine from
 *   d_c_in = the previous cycle's d_c_out, status in d_status_out)  ->  d_dm_out = C_occ C_occ^T  ->  J/K of d_dm_out,
 *   d_fock_out = d_hv + J - K[x], d_vhf_out = J - K[x]  ->  [want_grad: sum of squares of the virtual-occupied block of
 *   C^T F_out C per spin]  ->  scalars.
 * h_out (pinned, device-mapped host memory; the caller clears the last word and polls it):
 *   tr[(h + vhf/2) D] alpha, beta (their sum + E_nuc = energy_tot), |D - D_in|_F alpha, beta, the eigensolver's two
 *   status words (as nbx_huz_cycle), [want_grad: the two gradient sums], 1.0  -- 7 or 9 doubles.
 * Same kernels, order and operands as issuing the steps one by one: bit-identical results.                        */
int nbx_mu_cycle(nbx_ctx* ctx, const nbx_huz_state* st, const double* d_dm_in, const double* d_fock_in,
                 const double* d_c_in, double* d_dm_out, double* d_fock_out, double* d_vhf_out, double* d_c_out,
                 double* d_v_out, double* d_w_out, int mode, int refine_iters, int diis_on, int diis_slot, int diis_nd,
                 int want_grad, double* h_out, int* d_status_out);
/* The pieces.  nbx_mu_cycle_solve: CDIIS -> eigenproblem -> density (no J/K).  nbx_mu_cycle_fock: J/K + Fock matrix of
 * d_dm on this rank's WHOLE tensor, gradient if d_c != NULL, scalars (mode: whose status words travel with them --
 * 0 the guarded solver's, 1 d_status_tracked, -1 none: h_out is then 5 or 7 doubles) -- alone it is the build of the
 * starting density and of the conv_check cycle.  Several ranks (SURVEY 8e, J/K row slabs): nbx_mu_cycle_solve,
 * nbx_huz_cycle_jk on the new density, the caller's all-reduce of st->d_jk, nbx_mu_cycle_fock_post.              */
int nbx_mu_cycle_solve(nbx_ctx* ctx, const nbx_huz_state* st, const double* d_dm_in, const double* d_fock_in,
                       const double* d_c_in, double* d_dm_out, double* d_c_out, double* d_v_out, double* d_w_out,
                       int mode, int refine_iters, int diis_on, int diis_slot, int diis_nd, int* d_status_out);
int nbx_mu_cycle_fock(nbx_ctx* ctx, const nbx_huz_state* st, const double* d_dm, const double* d_dm_old,
                      const double* d_c, double* d_fock_out, double* d_vhf_out, int mode, const int* d_status_tracked,
                      double* h_out);
int nbx_mu_cycle_fock_post(nbx_ctx* ctx, const nbx_huz_state* st, const double* d_dm, const double* d_dm_old,
                           const double* d_c, double* d_fock_out, double* d_vhf_out, int mode,
                           const int* d_status_tracked, double* h_out);

/* ------------------------------------------------------------------ exchange-correlation evaluation
 * (E_xc, v_xc) of a two-spin density matrix on the stored grid arrays -- what the reference gets from PySCF's
 * numint + libxc behind dft.UKS.get_veff (nbed/driver.py:155-191, 315-431, 845-852, 1138-1231): three passes,
 * csrc/xc.hip.  d_ao (npts, nao) AO values, d_dao (3, npts, nao) their gradients (nbx_eval_ao, transformed to the
 * working AOs by the caller), row-major; nothing is read back by these calls.
 * nbx_xc_rho:  d_rho (2, npts) and d_grad (2, 3, npts) of d_dm (2, nao, nao; symmetric): rho_x = diag(ao D_x ao^T),
 *   grad rho_x = 2 diag(ao D_x dao^T); c = ao D_x is formed tile by tile on the matrix cores for both spins and
 *   reduced against ao / dao in the epilogue (each array read once).  nao <= 640.
 * nbx_xc_functional:  energy density and first derivatives, written out analytically, of `code` (the semi-local part:
 *   NBX_XC_SLATER; _LDA_VWN_RPA = Slater + VWN(RPA); _LDA_VWN5 = Slater + VWN5, PySCF's default "lda,vwn"; _B3LYP =
 *   0.08 Slater + 0.72 B88 + 0.19 VWN(RPA) + 0.81 LYP, libxc's HYB_GGA_XC_B3LYP without its 0.2 exact exchange;
 *   _LDA_PW_MOD = Slater + Perdew-Wang 1992 (LDA_C_PW_MOD); _PBE = GGA_X_PBE + GGA_C_PBE; _PBEH = 0.75 GGA_X_PBE +
 *   GGA_C_PBE, HYB_GGA_XC_PBEH ("PBE0", Gaussian's PBE1PBE) without its 0.25 exact exchange; _BLYP = Slater + B88 +
 *   LYP; _B3LYP5 = _B3LYP with VWN5 in place of VWN(RPA), HYB_GGA_XC_B3LYP5), d_w
 *   (npts) the quadrature weights.  Densities are clamped from below at rho_floor / 2 and points with
 *   rho_a + rho_b <= rho_floor carry no weight.  Out: d_vr (2, npts) = w dE/drho_x; d_vec (2, 3, npts) =
 *   w (2 dE/dsigma_xx grad rho_x + dE/dsigma_ab grad rho_other); d_sums[0] = E_xc, d_sums[1] = the integrated
 *   electron count (summed in a fixed order).  d_work: nbx_xc_functional_worksize() bytes.
 * nbx_xc_vmat:  d_vxc (2, nao, nao) = V + V^T, V_x[m][n] = sum_g ao[g][m] (d_vr[x][g] / 2 ao[g][n] + sum_a
 *   d_vec[x][a][g] dao[a][g][n]); the second factor is built on the fly as an operand of the product.  Split over
 *   chunks of grid points whose partial matrices are added in a fixed order.  d_work: nbx_xc_vmat_worksize() bytes. */
#define NBX_XC_SLATER 0
#define NBX_XC_LDA_VWN_RPA 1
#define NBX_XC_LDA_VWN5 2
#define NBX_XC_B3LYP 3
#define NBX_XC_LDA_PW_MOD 4
#define NBX_XC_PBE 5
#define NBX_XC_PBEH 6
#define NBX_XC_BLYP 7
#define NBX_XC_B3LYP5 8
/* nbx_xc_functional_rs: the semi-local part of a range-separated hybrid (what libxc evaluates behind dft.UKS.get_veff,
 * nbed/driver.py:155-191, when xc_functional names one), nbx_xc_functional's arguments and outputs plus the range
 * separation omega >= 0 (NBX_E_INVALID otherwise, and for every code but these two; nbx_xc_functional refuses them):
 *   NBX_XC_CAM_B3LYP = 0.35 (Slater + B88) + 0.46 B88^sr(omega) + 0.81 LYP + 0.19 VWN5 (Yanai, Tew and Handy, Chem. Phys.
 *     Lett. 393, 51 (2004): alpha = 0.19, beta = 0.46, omega = 0.33; exact part 0.19 K + 0.46 K_lr(omega), the caller's)
 *   NBX_XC_LC_BLYP   = B88^sr(omega) + LYP (exact part K_lr(omega))
 * B88^sr: the B88 exchange of a spin channel, Slater part and gradient correction together, times the attenuation
 * factor F(a) of Iikura, Tsuneda, Yanai and Hirao (J. Chem. Phys. 115, 3540 (2001)), a = omega / (2 k_sigma),
 * k_sigma = sqrt(9 pi / K_sigma) rho_sigma^(1/3) for e_sigma = -1/2 rho_sigma^(4/3) K_sigma; F by its closed form below
 * a = 1/2 and by its series in 1 / a^2 from there on.                                          */
#define NBX_XC_CAM_B3LYP 16
#define NBX_XC_LC_BLYP 17
int nbx_xc_functional_rs(nbx_ctx* ctx, int code, double omega, int64_t npts, const double* d_rho, const double* d_grad,
                         const double* d_w, double rho_floor, double* d_vr, double* d_vec, double* d_sums, void* d_work,
                         size_t work_bytes);
/* Meta-GGAs: the same three passes with the kinetic-energy density tau_x = 1/2 sum_i |grad psi_i|^2 carried through
 * them (what libxc evaluates behind dft.UKS.get_veff, nbed/driver.py:155-191, 315-431, 845-852, 1138-1231, when
 * xc_functional names a meta-GGA).  Entry points of their own: the ones above keep their arguments and their codes.
 * nbx_xc_rho_tau:  nbx_xc_rho plus d_tau (2, npts), tau_x = 1/2 sum_a diag(dao_a D_x dao_a^T).  For every 16-column tile
 *   the slab of D is staged in LDS once and multiplied by the fragments of ao and of each dao_a in turn, each product
 *   reduced in the epilogue against its own operand; d_rho and d_grad come out bit for bit as nbx_xc_rho's.  nao <= 640
 *   (NBX_E_UNSUPPORTED beyond).
 * nbx_xc_functional_mgga:  nbx_xc_functional's arguments plus d_tau (2, npts) in and d_vt (2, npts) = w dE/dtau_x out.
 *   NBX_XC_TPSS = TPSS exchange + TPSS correlation (Tao, Perdew, Staroverov and Scuseria, Phys. Rev. Lett. 91, 146401
 *   (2003)); NBX_XC_TPSSH = 0.9 TPSS exchange + TPSS correlation (Staroverov, Scuseria, Tao and Perdew, J. Chem. Phys.
 *   119, 12129 (2003)) without its 0.1 exact exchange.  Every other code: NBX_E_INVALID (and nbx_xc_functional /
 *   nbx_xc_functional_rs refuse these two).  Conventions besides nbx_xc_functional's: wherever z = tau_W / tau is formed,
 *   tau is clamped from below at tau_W = sigma / (8 n) of the same clamped quantities -- each spin channel's own in the
 *   exchange, the totals in the correlation -- by the float64 test tau >= sigma / (8 n) * (1 - 1e-10); where it fails
 *   z = 1 and alpha = 0 are constants (the margin: a one-orbital density sits on the clamp at every point, and the
 *   potential has a kink there).  "The larger of" eps_PBE(n_s, 0, grad n_s, 0) and eps_PBE is the first where it is >= the
 *   second.  DESIGN.md section 18.
 * nbx_xc_vmat_tau:  nbx_xc_vmat with the products sum_a dao_a^T (d_vt[x] / 4 dao_a) added to V_x before V + V^T (after
 *   it: 1/2 int v_tau grad phi_m . grad phi_n); with d_vt = 0 the result is nbx_xc_vmat's bit for bit.  d_work:
 *   nbx_xc_vmat_tau_worksize() bytes. */
#define NBX_XC_TPSS 32
#define NBX_XC_TPSSH 33
int nbx_xc_rho_tau(nbx_ctx* ctx, int64_t npts, int64_t nao, const double* d_ao, const double* d_dao, const double* d_dm,
                   double* d_rho, double* d_grad, double* d_tau);
int nbx_xc_functional_mgga(nbx_ctx* ctx, int code, int64_t npts, const double* d_rho, const double* d_grad,
                           const double* d_tau, const double* d_w, double rho_floor, double* d_vr, double* d_vec, double* d_vt,
                           double* d_sums, void* d_work, size_t work_bytes);
size_t nbx_xc_vmat_tau_worksize(int64_t npts, int64_t nao);
int nbx_xc_vmat_tau(nbx_ctx* ctx, int64_t npts, int64_t nao, const double* d_ao, const double* d_dao, const double* d_vr,
                    const double* d_vec, const double* d_vt, double* d_vxc, void* d_work, size_t work_bytes);
int nbx_xc_rho(nbx_ctx* ctx, int64_t npts, int64_t nao, const double* d_ao, const double* d_dao, const double* d_dm,
               double* d_rho, double* d_grad);
size_t nbx_xc_functional_worksize(int64_t npts);
int nbx_xc_functional(nbx_ctx* ctx, int code, int64_t npts, const double* d_rho, const double* d_grad, const double* d_w,
                      double rho_floor, double* d_vr, double* d_vec, double* d_sums, void* d_work, size_t work_bytes);
size_t nbx_xc_vmat_worksize(int64_t npts, int64_t nao);
int nbx_xc_vmat(nbx_ctx* ctx, int64_t npts, int64_t nao, const double* d_ao, const double* d_dao, const double* d_vr,
                const double* d_vec, double* d_vxc, void* d_work, size_t work_bytes);

/* ------------------------------------------------------------------ quadrature grid producers
 * What the reference gets from PySCF behind scf.UKS(...) (nbed/driver.py:86-104,315-431): `dft.gen_grid`'s Becke
 * partition and `numint.eval_ao`.  Inputs of the exchange-correlation part of V_emb (driver.py:845-852), not of
 * the SCF hot path; both one thread per grid point.
 * nbx_becke_share: d_share[g] = w_owner / sum_i w_i of Becke's cell functions (three smoothing iterations, size
 *   adjustment a_ij given by the caller) at the points d_pts (npts,3); d_centres (natm,3), d_aij and
 *   d_inv_dist = 1 / |R_i - R_j| (any finite value on the diagonal) are (natm,natm) (kept in LDS up to 96 atoms).
 * nbx_eval_ao: values d_out (npts, ncart) and, if d_dout != NULL, gradients (3, npts, ncart) of the contracted
 *   Cartesian Gaussians x^l y^m z^n sum_k c_k exp(-a_k r^2), l + m + n <= 3.  d_shell_i (nshell,4) =
 *   {first component, components, first primitive, primitives}; d_shell_centre (nshell,3); d_comp_lmn (ncart,4)
 *   = {l, m, n, offset of the component's coefficients in d_coefs}; max_prim = the largest primitive count
 *   (<= 24, NBX_E_UNSUPPORTED beyond).  The spherical transform is the caller's GEMM.               */
int nbx_becke_share(nbx_ctx* ctx, int64_t npts, const double* d_pts, int64_t natm, const double* d_centres,
                    const double* d_aij, const double* d_inv_dist, int64_t owner, double* d_share);
int nbx_eval_ao(nbx_ctx* ctx, int64_t npts, const double* d_pts, int64_t nshell, const int* d_shell_i,
                const double* d_shell_centre, const int* d_comp_lmn, const double* d_exps, const double* d_coefs,
                int64_t ncart, int64_t max_prim, double* d_out, double* d_dout);
/* ------------------------------------------------------------------ density by purification
 * The projector P on the nocc LOWEST eigenvectors of each symmetric matrix d_f (batch, n, n; an orthonormal
 * basis), i.e. C_occ C_occ^T of `eigh` + aufbau occupation (nbed/scf/huzinaga_scf.py:166-174) without the
 * eigenvectors: trace-correcting purification (SP2), one (n x n) product per step, everything decided on
 * the device.  For SCF cycles whose Fock matrix still moves too much for a warm-started eigensolver.
 *   nocc_a, nocc_b : occupied levels of matrix 0 and of the others (batch = 2: alpha, beta); a batch of more
 *                    than two needs nocc_a == nocc_b (NBX_E_INVALID otherwise)
 *   d_p            : out (batch, n, n)
 *   d_work         : nbx_purify_worksize() bytes;  max_iter <= 0: the limit (72 steps)
 *   d_status[b]    : > 0 steps taken; < 0 no gap between levels nocc and nocc + 1 was resolved (or the
 *                    matrix is not finite): d_p is then meaningless                                      */
size_t nbx_purify_worksize(int64_t n, int64_t batch);
int nbx_purify(nbx_ctx* ctx, int64_t n, int64_t batch, const double* d_f, int64_t nocc_a, int64_t nocc_b, double* d_p,
               void* d_work, size_t work_bytes, int max_iter, int* d_status);

/* d_x[i] <- (|d_x[i]| < tol ? 0 : d_x[i]) * scale over n doubles: the 1e-8 truncation
 * (nbed/ham_builder.py:213-214) and the 1/2 of build() (:254) applied to a SPATIAL block, for callers
 * that keep the three unique spin blocks (aaaa, bbbb, aabb) instead of the 16x larger scattered
 * spin-orbital tensor.                                                                          */
int nbx_threshold_scale(nbx_ctx* ctx, int64_t n, double tol, double scale, double* d_x);

/* ------------------------------------------------------------------ AO integrals of a real molecule (HOST)
 * (pq|rs) over contracted Gaussian shells of angular momentum <= 3, dense (nao, nao, nao, nao) in HOST
 * memory: the producer the reference reaches through PySCF/libcint (gto.Mole.intor("int2e"), implied by
 * scf.UKS(mol).kernel() at nbed/driver.py:155-191 and ao2mo at nbed/ham_builder.py:139-170).  Input of
 * the hot path, produced once per molecule: host threads, no GPU, no context.
 *   ang, nprim, nfunc (nshell)   angular momentum, primitive count, AO count (2l+1, or (l+1)(l+2)/2
 *                                to keep the Cartesian components) of each shell
 *   centres (nshell, 3)          Bohr
 *   exps, coefs                  primitives of all shells, concatenated; coefs carry the radial
 *                                normalisation (common to the components of a shell)
 *   sph                          per shell a (nfunc, ncart) matrix from the Cartesian components
 *                                (xx xy xz yy yz zz; xxx xxy xxz xyy xyz xzz yyy yyz yzz zzz)
 *                                to its AOs, concatenated; only read for l >= 2
 *   cutoff                       Schwarz bound below which a shell quartet is skipped (1e-16: below fp64
 *                                resolution of the O(1) integrals)
 *   nthreads                     <= 0: all hardware threads                                              */
int nbx_host_eri(int nshell, const int* ang, const int* nprim, const int* nfunc, const double* centres,
                 const double* exps, const double* coefs, const double* sph, double cutoff, int nthreads,
                 double* out);
/* The same tensor over the attenuated operator, (pq| erf(omega r12) / r12 |rs): the long-range integrals of a
 * range-separated hybrid (mol.intor("int2e") under mol.with_range_coulomb(omega), what PySCF's get_veff asks for when
 * xc_functional -- handed over untouched at nbed/driver.py:155-191 -- names one).  Per primitive quartet with
 * alpha = p q / (p + q) it is the plain integral at alpha_w = alpha omega^2 / (alpha + omega^2), in the Boys argument
 * and in the powers (-2 alpha_w)^n, times omega / sqrt(alpha + omega^2); nbx_host_eri is its omega = infinity case and
 * runs the same code.  The quartets skipped are nbx_host_eri's: the Schwarz bounds of 1 / r12 bound the attenuated
 * integrals too.  omega finite and > 0, else NBX_E_INVALID.                                                          */
int nbx_host_eri_erf(int nshell, const int* ang, const int* nprim, const int* nfunc, const double* centres,
                     const double* exps, const double* coefs, const double* sph, double cutoff, double omega,
                     int nthreads, double* out);
/* Overlap, kinetic-energy and nuclear-attraction matrices (nao, nao) of the same shells, HOST memory:
 * intor("int1e_ovlp"), ("int1e_kin"), ("int1e_nuc") behind get_ovlp() / get_hcore() (nbed/driver.py:155-191).
 *   charges (natm), atom_xyz (natm, 3): the point charges of V (nuclei; Bohr)                      */
int nbx_host_1e(int nshell, const int* ang, const int* nprim, const int* nfunc, const double* centres,
                const double* exps, const double* coefs, const double* sph, int natm, const double* charges,
                const double* atom_xyz, int nthreads, double* s_out, double* t_out, double* v_out);
/* Dipole matrices <mu| r |nu> (3, nao, nao) of the same shells, origin at 0, HOST memory: intor_symmetric("int1e_r",
 * comp=3) behind pyscf.lo.boys (nbed/localizers/occupied/pyscf.py:378).  <a|x|b> = (E_1 + P_x E_0) (pi/p)^1/2 times
 * the y and z overlap factors.                                                                        */
int nbx_host_dipole(int nshell, const int* ang, const int* nprim, const int* nfunc, const double* centres,
                    const double* exps, const double* coefs, const double* sph, int nthreads, double* r_out);

/* ------------------------------------------------------------------ AO integrals of a real molecule (DEVICE)
 * The same tensor as nbx_host_eri, dense (nao, nao, nao, nao), written into DEVICE memory by csrc/eri.hip: the
 * producer the reference reaches through PySCF/libcint (gto.Mole.intor("int2e"), implied by
 * scf.UKS(mol).kernel() at nbed/driver.py:155-191 and ao2mo at nbed/ham_builder.py:139-170), without the host
 * tensor and its upload.  The shell arguments are nbx_host_eri's HOST arrays; pair data, primitive screening
 * (cutoff * 1e-4) and the Schwarz test are the host engine's own code (csrc/ints_md.h), so both engines skip the
 * same quartets and differ only in rounding.  Shells of angular momentum <= 2 (NBX_E_INVALID for l = 3: f shells
 * stay on nbx_host_eri, and wherever nbx_host_eri refuses the shells).
 *   out_device   nao^4 doubles; zeroed and filled on the context's stream (one launch per non-empty class
 *                (la + lb, lc + ld), no atomics: two calls give the same bits).  The call returns once the pair
 *                data and quartet lists have left host memory; the launches are queued behind them.
 * While profiling is enabled for NBX_PROF_ERI every class launch is bracketed by HIP events;
 * nbx_eri_class_ms waits for those of the last call and returns milliseconds per class (index 5 (la + lb) +
 * (lc + ld), 0 for an empty class).                                                                          */
#define NBX_PROF_ERI 7
#define NBX_ERI_CLASSES 25
int nbx_eri_device(nbx_ctx* ctx, int nshell, const int* ang, const int* nprim, const int* nfunc, const double* centres,
                   const double* exps, const double* coefs, const double* sph, double cutoff, double* out_device);
/* nbx_eri_device_erf: the tensor of nbx_host_eri_erf, (pq| erf(omega r12) / r12 |rs) (mol.with_range_coulomb(omega)
 * around the intor("int2e") of nbed/driver.py:155-191), by the same class kernel: omega travels with the kernel's
 * arguments, nbx_eri_device is the omega = infinity case.  Quartet lists, launches (nbx_eri_plan answers for every
 * omega), storing rule, profiling and refusals as nbx_eri_device; omega finite and > 0, else NBX_E_INVALID.         */
int nbx_eri_device_erf(nbx_ctx* ctx, int nshell, const int* ang, const int* nprim, const int* nfunc,
                       const double* centres, const double* exps, const double* coefs, const double* sph, double cutoff,
                       double omega, double* out_device);
int nbx_eri_class_ms(nbx_ctx* ctx, double* ms_out);
/* Test support and launch geometry of nbx_eri_device -- the function its launcher asks, host arithmetic only (no
 * context, no GPU; the intor("int2e") call of nbed/driver.py:155-191 has no counterpart of it).  Per class
 * (index 5 (la + lb) + (lc + ld), NBX_ERI_CLASSES entries each):
 *   counts_out      canonical shell quartets (kl <= ij) that pass the Schwarz test; 0 = nothing is launched
 *   lds_bytes_out   static LDS of one workgroup of the class's kernel
 *   block_out       threads per workgroup (one wavefront, which owns one quartet at a time)
 *   grid_out        workgroups launched (they stride over the class's list)
 * NBX_E_INVALID exactly where nbx_eri_device returns it.                                                      */
int nbx_eri_plan(int nshell, const int* ang, const int* nprim, const int* nfunc, const double* centres,
                 const double* exps, const double* coefs, const double* sph, double cutoff, int64_t* counts_out,
                 int* lds_bytes_out, int* block_out, int64_t* grid_out);

/* ------------------------------------------------------------------ (pq|rs) of a real molecule without the tensor
 * The same integrals -- gto.Mole.intor("int2e") behind scf.UKS(mol).kernel() at nbed/driver.py:155-191 -- asked for by
 * the diagonal and by columns, and their pivoted incomplete Cholesky factor (pq|rs) ~ sum_L B_L[pq] B_L[rs], the input
 * of nbx_jk_df (get_veff at nbed/scf/huzinaga_scf.py:156), DESIGN.md section 13.  The N^4 tensor is never formed.  Shell
 * arguments, cutoff and screening as nbx_eri_device (the same class kernel with another last stage), and the same
 * refusals: NBX_E_INVALID for l > 2 and wherever nbx_host_eri refuses the shells.  No atomics, one writer per address:
 * two calls give the same bits, and a value is the same double wherever it is stored.
 *
 * nbx_eri_diagonal: d_diag[p][q] = d_diag[q][p] = (pq|pq), (nao, nao), zeroed and filled on the context's stream.    */
int nbx_eri_diagonal(nbx_ctx* ctx, int nshell, const int* ang, const int* nprim, const int* nfunc, const double* centres,
                     const double* exps, const double* coefs, const double* sph, double cutoff, double* d_diag);
/* nbx_eri_columns (the intor("int2e") of nbed/driver.py:155-191, a column at a time): the shell pairs (ia[k] >= ib[k]),
 * k < npair, select the columns m = the function pairs (r >= s) of pair 0, then of pair 1, ..., (r, s) row-major
 * within a pair; d_cols[m][p][q] = d_cols[m][q][p] = (pq|rs), (ncols, nao, nao), zeroed and filled on the context's
 * stream (quartets the Schwarz test drops stay zero).  The values are those of nbx_eri_device, bit for bit, and do not
 * depend on which other pairs are listed.                                                                       */
int nbx_eri_columns(nbx_ctx* ctx, int nshell, const int* ang, const int* nprim, const int* nfunc, const double* centres,
                    const double* exps, const double* coefs, const double* sph, double cutoff, int npair, const int* ia,
                    const int* ib, double* d_cols);
/* nbx_eri_cholesky (intor("int2e") at nbed/driver.py:155-191 in the factorised form get_veff at
 * nbed/scf/huzinaga_scf.py:156 can contract): shell-blocked pivoted Cholesky, host driven with one small read-back per step.
 *   tol         stop when the largest residual diagonal is <= tol; then |(pq|rs) - sum_L B_L[pq] B_L[rs]| <= tol for
 *               every element (the residual is positive semi-definite).  Finite and >= 1e-12, else NBX_E_INVALID.
 *   max_rank    >= 1 (else NBX_E_INVALID): room of d_b in slices.  Reaching it first is not an error: *resid_out > tol.
 *   d_b         (max_rank, nao, nao) DEVICE: slices [0, *rank_out) are written, each symmetric bit for bit (the input
 *               format of nbx_jk_df); the others, and all of it when the call is refused, are left untouched.
 *   rank_out, resid_out   HOST: vectors written; largest remaining residual diagonal.
 * The call returns with the stream idle.                                                                        */
int nbx_eri_cholesky(nbx_ctx* ctx, int nshell, const int* ang, const int* nprim, const int* nfunc, const double* centres,
                     const double* exps, const double* coefs, const double* sph, double cutoff, double tol,
                     int64_t max_rank, double* d_b, int64_t* rank_out, double* resid_out);
/* Host bookkeeping of the last nbx_eri_cholesky call on this thread (the intor("int2e") call of
 * nbed/driver.py:155-191 has no counterpart of it): steps taken and columns (pq|m) computed.                 */
int nbx_eri_cholesky_steps(int64_t* steps, int64_t* columns);

/* ------------------------------------------------------------------ potential of an MM environment (QM/MM)
 * What qmmm.mm_charge(mf, coords, charges, radii) adds to get_hcore() of the objects the reference wraps
 * (nbed/driver.py:171-180 global Kohn-Sham, :246-253 embedded HF), over the shells of nbx_host_eri:
 *   V[mu][nu] = - sum_c q_c int mu(r) nu(r) erf(sqrt(zeta_c) |r - C_c|) / |r - C_c| dr,    zeta_c = 1 / radius_c^2,
 * the potential of normalised Gaussian charges; zeta == NULL: point charges (int1e_nuc with the charges as nuclei).
 *   q (ncharge), xyz (ncharge, 3; Bohr), zeta (ncharge, > 0, or NULL)   HOST arrays, finite
 * nbx_host_mm_potential: shells of l <= 3, v_out (nao, nao) HOST, every element written (zeros for ncharge = 0),
 * exactly symmetric, independent of nthreads (<= 0: all hardware threads); no primitive pair is screened.         */
int nbx_host_mm_potential(int nshell, const int* ang, const int* nprim, const int* nfunc, const double* centres,
                          const double* exps, const double* coefs, const double* sph, int ncharge, const double* q,
                          const double* xyz, const double* zeta, int nthreads, double* v_out);
/* nbx_mm_potential (the same addition to get_hcore(), nbed/driver.py:171-180, 246-253, on the device; csrc/mm_potential.hip,
 * DESIGN.md section 15): shells, cutoff, primitive screening (cutoff * 1e-4) and refusals as nbx_eri_diagonal
 * (NBX_E_INVALID for l > 2); one upload of the charges.  v_device (nao, nao) DEVICE: every element written (exact zeros
 * where all primitive pairs of a shell pair are screened out, and for ncharge = 0), exactly symmetric.  No atomics;
 * the order of every sum depends on the shells and on ncharge alone: two calls give the same bits.  The call returns
 * with the stream idle.                                                                                            */
int nbx_mm_potential(nbx_ctx* ctx, int nshell, const int* ang, const int* nprim, const int* nfunc, const double* centres,
                     const double* exps, const double* coefs, const double* sph, double cutoff, int ncharge,
                     const double* q, const double* xyz, const double* zeta, double* v_device);

/* ------------------------------------------------------------------ four-index transform from a factor
 * The three ao2mo.kernel calls of nbed/ham_builder.py:127-133 (aaaa, bbbb, aabb; C1 = C2 and C3 = C4 in each) computed
 * from the factor of nbx_eri_cholesky instead of the N^4 tensor (csrc/ao2mo_factor.hip):
 *   M_L^x = C_x^T B_L C_x,   (ij|kl)_xy = sum_L M_L^x[i][j] M_L^y[k][l].
 *   d_b          (naux, nao, nao) DEVICE, every slice symmetric; naux >= 1
 *   nset         1 (one matrix d_ca: one block d_aaaa; d_cb, d_bbbb, d_aabb NULL) or 2 (aaaa, bbbb, aabb)
 *   d_ca, d_cb   (nao, n) row-major with leading dimensions ldca, ldcb >= n (column slices of a wider matrix are fine)
 *   d_aaaa ...   (n, n, n, n) chemist order, every element written; (ij|kl), (ji|kl), (ij|lk), (ji|lk) are the same double
 *   d_work       nbx_ao2mo_factor_worksize() bytes: the packed half transform P and one (npair x npair) product,
 *                npair = n (n + 1) / 2.  0 from the worksize call = arguments the transform refuses.
 * Stages: nbx_ao2mo_factor_half (P[x][L][i (i + 1) / 2 + j] = M_L^x[i][j], j <= i: (nset, naux, npair), the intermediate
 * B_L C kept on chip, fp64 MFMA), nbx_gemm 'T','N' over L, nbx_ao2mo_factor_expand (out[i][j][k][l] =
 * G[pair(i,j)][pair(k,l)] of an (npair x npair) matrix G, a copy).  No atomics, fixed summation order: two calls give the
 * same bits.  NBX_E_UNSUPPORTED for n > 361 (more than 65535 pairs, as nbx_ao2mo_pair_sym); NBX_E_INVALID for naux < 1
 * and bad shapes, NBX_E_NOMEM for a short workspace: a refused call writes nothing.                                  */
size_t nbx_ao2mo_factor_worksize(int64_t nao, int64_t naux, int64_t n, int64_t nset);
int nbx_ao2mo_factor(nbx_ctx* ctx, int64_t nao, int64_t naux, const double* d_b, int64_t nset, const double* d_ca,
                     int64_t ldca, const double* d_cb, int64_t ldcb, int64_t n, double* d_aaaa, double* d_bbbb,
                     double* d_aabb, void* d_work, size_t work_bytes);
int nbx_ao2mo_factor_half(nbx_ctx* ctx, int64_t nao, int64_t naux, const double* d_b, int64_t nset, const double* d_ca,
                          int64_t ldca, const double* d_cb, int64_t ldcb, int64_t n, double* d_p);
int nbx_ao2mo_factor_expand(nbx_ctx* ctx, int64_t n, const double* d_g, double* d_out);

/* ------------------------------------------------------------------ coupled cluster (csrc/ccsd.hip)
 * What surrounds the GEMMs of a spin-orbital CCSD (nbed_amd/ccsd_gpu.py): the reference runs PySCF's
 * cc.CCSD on the embedded object (nbed/driver.py:1105-1135); here the amplitude equations of
 * nbed_amd/ccsd.py run on the device with every contraction an nbx_gemm.  Spin orbital 2p + s has
 * spatial orbital p and spin s (alpha = 0): the convention of nbx_spinorb_scatter.  None of these
 * synchronises.
 *
 * Antisymmetrised block  out[a,b,c,d] = <P Q || R S>,  P = idx1[a], Q = idx2[b], R = idx3[c], S = idx4[d],
 * of the Hamiltonian whose spatial blocks are d_two_body (3, n, n, n, n): aaaa, bbbb, aabb in physicist
 * order, truncated and halved as build_spatial() leaves them (nbx_threshold_scale).  With h2 the
 * spin-orbital tensor of build() -- h2[P,Q,R,S] is block aaaa / bbbb / aabb[p,q,r,s] / aabb[q,p,s,r] for
 * the spins (a,a,a,a) / (b,b,b,b) / (a,b,b,a) / (b,a,a,b) and zero otherwise -- and w[P,Q,R,S] = 2 h2[P,Q,S,R],
 *      <PQ||RS> = 0.5 ((w[P,Q,R,S] - w[P,Q,S,R]) - (w[Q,P,R,S] - w[Q,P,S,R])),
 * the four terms of nbed_amd.ccsd.antisymmetrized in its order.  The (2n)^4 tensor is never formed.
 *   pack_last  != 0: idx3 and idx4 are the same list and only c < d is written, as pair index
 *                    c (2 n3 - c - 1) / 2 + (d - c - 1); pack_first: the same for a < b.
 *   d_idx*         : device int arrays of spin-orbital indices in [0, 2n)                          */
int nbx_ccsd_gather(nbx_ctx* ctx, int64_t n, const double* d_two_body, const int* d_idx1, int64_t n1,
                    const int* d_idx2, int64_t n2, const int* d_idx3, int64_t n3, const int* d_idx4, int64_t n4,
                    int pack_first, int pack_last, double* d_out);
/* Fock matrix of the determinant that occupies the spin orbitals d_occ (nocc ints), over all 2n spin
 * orbitals: f[P,Q] = h1[P,Q] + sum_I <P I || Q I>, d_h1 and d_fock (2n, 2n); the mean field the CCSD of
 * nbed/driver.py:1105-1135 starts from, without a (2n)^4 tensor.                                  */
int nbx_ccsd_fock(nbx_ctx* ctx, int64_t n, const double* d_two_body, const double* d_h1, const int* d_occ,
                  int64_t nocc, double* d_fock);
/* out = alpha * transpose(in, perm) + beta * out for a four-index tensor: h_extents (4) are the extents of
 * `in`, output axis k is input axis h_perm[k] (numpy.transpose), any of the 24 permutations, any extents
 * (lower ranks: leading extents of 1).  beta == 0: `out` is not read.  The permutes that turn a contraction
 * of the CCSD equations (nbed/driver.py:1105-1135) into a matrix product, and with beta = 1 the P(ij),
 * P(ab) antisymmetrisations of the doubles residual.  Tiled through LDS when the fastest axis changes.  */
int nbx_permute4(nbx_ctx* ctx, const int64_t* h_extents, const int* h_perm, double alpha, const double* d_in,
                 double beta, double* d_out);
/* Antisymmetric index pairs of the CCSD tensors (nbed/driver.py:1105-1135): x (lead, n, n, trail) with
 * x[l,e,f,t] = -x[l,f,e,t] against packed (lead, n(n-1)/2, trail) over e < f, pair index
 * e (2n - e - 1) / 2 + (f - e - 1).  pack reads the e < f element; unpack writes
 * x = alpha * (+packed | -packed | 0 on the diagonal) + beta * x  (beta == 0: x is not read).       */
int nbx_pair_pack(nbx_ctx* ctx, int64_t lead, int64_t n, int64_t trail, const double* d_x, double* d_packed);
int nbx_pair_unpack(nbx_ctx* ctx, int64_t lead, int64_t n, int64_t trail, double alpha, const double* d_packed,
                    double beta, double* d_x);
/* out[i,j,a,b] = c_t2 t2[i,j,a,b] + c_direct t1[i,a] t1[j,b] - c_exchange t1[i,b] t1[j,a]: tau (1, 1, 1),
 * tau~ (1, 1/2, 1/2) and the 1/2 t2 + t1 t1 of W_mbej (1/2, 1, 0) of the CCSD equations
 * (nbed/driver.py:1105-1135).  packed != 0: out is (nocc(nocc-1)/2, nvir(nvir-1)/2) over i < j, a < b.  */
int nbx_ccsd_tau(nbx_ctx* ctx, int64_t nocc, int64_t nvir, const double* d_t1, const double* d_t2, double c_t2,
                 double c_direct, double c_exchange, int packed, double* d_out);
/* Amplitude update of a CCSD cycle (nbed/driver.py:1105-1135) over the concatenated [t1 | t2] vector of
 * nocc nvir + (nocc nvir)^2 doubles: t_new = r / D with D_ia = eo[i] - ev[a], D_ijab = eo[i] + eo[j] - ev[a]
 * - ev[b] (the occupied / virtual Fock diagonals), err = t_new - t_old, and max |err| (NaN if any is) into the
 * device double d_maxerr.  d_t_new and d_err are typically a slot of the DIIS history.              */
int nbx_ccsd_update(nbx_ctx* ctx, int64_t nocc, int64_t nvir, const double* d_r, const double* d_t_old,
                    const double* d_eo, const double* d_ev, double* d_t_new, double* d_err, double* d_maxerr);
/* Lambda equations and density (csrc/ccsd_lambda.hip): what nbed_amd/ccsd_gpu.py needs besides GEMMs and permutes
 * to give the CCSD of nbed/driver.py:1105-1135 its left-hand state and one-particle density.
 *
 * Disconnected term of the doubles Lambda equation, in one pass over d_r2 (nocc, nocc, nvir, nvir):
 *      r2[i,j,a,b] += alpha ( x[i,a] y[j,b] - x[j,a] y[i,b] - x[i,b] y[j,a] + x[j,b] y[i,a] ),
 * x and y (nocc, nvir), or (nvir, nocc) where the bit of `layout` is set (bit 0: x, bit 1: y).  Grid-stride, no
 * atomics.  Does not synchronise.                                                                           */
int nbx_ccsd_lambda_outer(nbx_ctx* ctx, int64_t nocc, int64_t nvir, double alpha, const double* d_x, const double* d_y,
                          int layout, double* d_r2);
/* Spin-resolved, symmetrised one-particle density d_dm1 (2, n, n), dm1[s,p,q] = <a+_{p s} a_{q s}>, in the original
 * orbital order from its blocks over occupied / virtual spin orbitals: d_goo (nocc, nocc), d_gov (nocc, nvir), d_gvo
 * (nvir, nocc), d_gvv (nvir, nvir), with d_occ and d_vir (device ints; together a permutation of [0, 2n), which the
 * caller guarantees: every element of d_dm1 is then written once).  dm1 = 1/2 (gamma + gamma^T) + the occupations of
 * the reference determinant.  The max |gamma[P,Q]| over pairs of different spins -- zero for a Hamiltonian of the
 * spin-block form -- goes to the device double d_cross (NaN if any is).  One workgroup, no atomics.  Does not
 * synchronise.                                                                                              */
int nbx_ccsd_rdm1(nbx_ctx* ctx, int64_t n, int64_t nocc, int64_t nvir, const int* d_occ, const int* d_vir,
                  const double* d_goo, const double* d_gov, const double* d_gvo, const double* d_gvv, double* d_dm1,
                  double* d_cross);
/* Perturbative triples (csrc/ccsd_t.hip): the (T) a PySCF user adds with ccsd_t() to the CCSD of
 * nbed/driver.py:1105-1135, in the non-HF form (f_ov != 0) over semicanonical spin orbitals (f_oo, f_vv
 * diagonal: d_eo, d_ev).  d_cubes holds ncubes <= 65535 cubes W (nvir, nvir, nvir), cube x that of the
 * occupied triple i < j < k = d_ijk[3x .. 3x+2] (device ints, trusted), built by the caller with nbx_gemm:
 *      W[a,b,c] = P(i/jk) [ sum_e t2[j,k,a,e] <ei||bc> - sum_m t2[i,m,b,c] <ma||jk> ],
 *      P(p/qr) g(pqr) = g(pqr) - g(qpr) - g(rqp).
 * For every a < b < c the kernel forms w = W[a,b,c] - W[b,a,c] - W[c,b,a], the disconnected part
 *      t_d = P(i/jk) P(a/bc) [ t1[i,a] oovv[j,k,b,c] + fov[i,a] t2[j,k,b,c] ],
 * D = eo[i] + eo[j] + eo[k] - ev[a] - ev[b] - ev[c], and writes  sum_x sum_{a<b<c} w (w + t_d) / D  into the
 * device double d_energy.  The cube is tiled 16 (a) x 4 (b) x 16 (c) through LDS so that all three reads run
 * along the fastest index; nbx_ccsd_triples_tile() returns the 16.  No atomics: every workgroup writes its
 * partial sum into d_work (nbx_ccsd_triples_worksize bytes, every slot written) and one workgroup adds them in
 * a fixed order, so equal (nocc, nvir, ncubes) and inputs give equal bits.  nocc < 3, nvir < 3 or ncubes == 0:
 * d_energy = 0, nothing else launched.  NBX_E_NOMEM for a short workspace.  Does not synchronise.        */
size_t nbx_ccsd_triples_worksize(int64_t nvir, int64_t ncubes);
int nbx_ccsd_triples_tile(void);
int nbx_ccsd_triples_energy(nbx_ctx* ctx, int64_t nocc, int64_t nvir, int64_t ncubes, const double* d_cubes,
                            const int* d_ijk, const double* d_t1, const double* d_fov, const double* d_t2,
                            const double* d_oovv, const double* d_eo, const double* d_ev, void* d_work,
                            size_t work_bytes, double* d_energy);

/* ------------------------------------------------------------------ MP2 (csrc/mp2.hip)
 * Second-order amplitudes and pair energy of one spin pair: what a PySCF user gets from mp.MP2 / mp.UMP2 on
 * the embedded object the reference hands to its post-HF step (nbed/driver.py:1105-1135), in the non-canonical
 * form over semicanonical orbitals (f_oo, f_vv diagonal per spin: d_eo*, d_ev*).  d_v is the chemist block
 * V[i,a,j,b] = (ia|jb), row-major (no1, nv1, no2, nv2).  With d = ((eo1[i] + eo2[j]) - ev1[a]) - ev2[b],
 * evaluated in this order,
 *      same_spin == 0:  t = V[i,a,j,b] / d,                  energy = sum t V[i,a,j,b];
 *      same_spin != 0:  t = (V[i,a,j,b] - V[i,b,j,a]) / d,   energy = 1/4 sum t (V[i,a,j,b] - V[i,b,j,a]),
 * which needs nv1 == nv2 and no1 <= no2: no1 < no2 is a slice over i of the square block (rows i of V and of
 * d_eo1 those of the slice; the sum is then the slice's share).  a == b gives an exact 0.
 * d_t receives the amplitudes in the layout T[a, i, j, b], row-major (nv1, no1, no2, nv2), chosen so that both
 * virtual-virtual densities are one nbx_gemm on the buffer as it stands:
 *      D1[a,b] = sum_{ijc} t_iajc t_ibjc = T T^T   with T as (nv1) x (no1 no2 nv2):  'N','T';
 *      D2[c,d] = sum_{aij} t_iajc t_iajd = T^T T   with T as (nv1 no1 no2) x (nv2):  'T','N'.
 * A workgroup takes an (i, j) pair and a 32 x 32 tile of (a, b) -- nbx_mp2_pairs_tile() returns the 32 --; in
 * the same-spin case together with its mirror tile, both read along b and exchanged through LDS.  No atomics:
 * every workgroup writes the partial sum of the items it walked into d_work (nbx_mp2_pairs_worksize bytes, every
 * slot written) and one workgroup adds them in a fixed order, so equal shapes and inputs give equal bits.  Any
 * extent is legal; an empty block gives d_energy = 0 and launches nothing.  NBX_E_NOMEM for a short workspace.
 * Does not synchronise.                                                                                   */
size_t nbx_mp2_pairs_worksize(int64_t no1, int64_t nv1, int64_t no2, int64_t nv2, int same_spin);
int nbx_mp2_pairs_tile(void);
int nbx_mp2_pairs(nbx_ctx* ctx, int64_t no1, int64_t nv1, int64_t no2, int64_t nv2, const double* d_v,
                  const double* d_eo1, const double* d_ev1, const double* d_eo2, const double* d_ev2, int same_spin,
                  double* d_t, void* d_work, size_t work_bytes, double* d_energy);

/* ------------------------------------------------------------------ full CI (csrc/fci.hip)
 * What surrounds the GEMM of a determinant FCI sigma build (nbed_amd/fci_gpu.py): the reference runs PySCF's
 * fci.FCI on the embedded object (nbed/driver.py:1044-1102); here H c is formed on the device from the three
 * spatial spin blocks d_two_body (3, n, n, n, n) and d_one_body (2, n, n) of build_spatial().  A determinant is
 * (alpha string, beta string); strings are ranked lexicographically by their ascending lists of occupied
 * orbitals, the CI vector is row-major (n_alpha_str, n_beta_str), determinant indices are 64-bit.  With
 * E_ps = a+_p a_s,  a+_p a+_q a_r a_s = E_ps E_qr - delta_qs E_pr, so
 *      H = const + sum_g k_g E_g + sum_{g g'} G[g, g'] E_g E_g',     g = (spin, p, s) = spin n^2 + p n + s,
 *      G[(a,ps),(a,qr)] = aaaa[p,q,r,s], G[(b,ps),(b,qr)] = bbbb[p,q,r,s], G[(a,ps),(b,qr)] = aabb[p,q,r,s],
 *      G[(b,ps),(a,qr)] = aabb[q,p,s,r],  k_(s,pr) = one_body[s][p,r] - sum_q two_body[ss][p,q,r,q].
 * Link tables (int, built by the caller): link[S, k n + l] = sign (rank + 1) of E_kl |S>, 0 where it
 * vanishes; d_link_a is (n_alpha_str, n^2), d_link_bt the TRANSPOSED beta table (n^2, n_beta_str).  The kernels
 * trust them.  n <= 31, n_beta_str <= 13312 (a row is staged in LDS).  None of these synchronises.
 *
 * d_g (2 n^2, 2 n^2 + 1) = [G | k].                                                                     */
int nbx_fci_gmat(nbx_ctx* ctx, int64_t n, const double* d_one_body, const double* d_two_body, double* d_g);
/* d_d (2 n^2 + 1, rows n_beta_str): D[g, K] = <K| E_g |c> for the determinants K of alpha rows
 * [row0, row0 + rows), and c itself in the last row, so that E = d_g . d_d carries the k term.      */
int nbx_fci_gather(nbx_ctx* ctx, int64_t n, int64_t n_alpha_str, int64_t n_beta_str, int64_t row0, int64_t rows,
                   const int* d_link_a, const int* d_link_bt, const double* d_c, double* d_d);
/* sigma_I = (accumulate ? sigma_I : shift c_I) + sum_{g, K in the chunk} <I| E_g |K> E[g, K] over ALL I, d_e
 * (2 n^2, rows n_beta_str).  One gather per output element, summed in a fixed order, no atomics: the same
 * chunks in the same order give the same bits.                                                        */
int nbx_fci_scatter(nbx_ctx* ctx, int64_t n, int64_t n_alpha_str, int64_t n_beta_str, int64_t row0, int64_t rows,
                    const int* d_link_a, const int* d_link_bt, const double* d_e, double shift, const double* d_c,
                    int accumulate, double* d_sigma);
/* d_diag[I] = H_II = constant + sum_{P in I} h1[P,P] + sum_{P != Q in I} (h2[P,Q,Q,P] - h2[P,Q,P,Q]); d_str_a /
 * d_str_b: the bit masks of the ranked strings (the Davidson preconditioner of the solver that stands in for
 * fci.FCI.kernel, nbed/driver.py:1044-1102).                                                         */
int nbx_fci_diag(nbx_ctx* ctx, int64_t n, int64_t n_alpha_str, int64_t n_beta_str, const int* d_str_a,
                 const int* d_str_b, const double* d_one_body, const double* d_two_body, double constant,
                 double* d_diag);
/* Davidson correction out = r / (diag - theta), |diag - theta| < guard replaced by +-guard.         */
int nbx_fci_precond(nbx_ctx* ctx, int64_t ndet, double theta, double guard, const double* d_r, const double* d_diag,
                    double* d_out);

/* Densities (csrc/fci_rdm.hip): what PySCF's make_rdm1 / make_rdm12 / trans_rdm12 give the reference's users from the
 * fci.FCI object.  Between a bra b and a ket c of one sector, in the blocks and index order of d_two_body:
 *      dm1[s][p,q] = <b| a+_ps a_qs |c>,   dm2[x][p,q,r,s] = <b| a+_ps a+_qt a_rt a_ss |c>,  (s,t) = aa, bb, ab.
 * With D_x = nbx_fci_gather of x, Graw = D_b . D_c^T (nbx_gemm 'N','T') holds <b| E^s_lk E^t_mn |c> at
 * [(s,kl),(t,mn)], <b| E^s_lk |c> in its last column and <b|c> in its corner.
 *
 * d_graw (slabs, 2n^2 + 1, 2n^2 + 1): partial products over disjoint ranges of determinants; they are added in
 * ascending slab order, mapped to d_dm1 (2,n,n) and d_dm2 (3,n,n,n,n) with the delta_st delta_qs <b| E^s_pr |c>
 * subtracted, and <b|c> goes to d_overlap[0].  One thread per output element, every element written.           */
int nbx_fci_rdm_finish(nbx_ctx* ctx, int64_t n, int64_t slabs, const double* d_graw, double* d_dm1, double* d_dm2,
                       double* d_overlap);
/* d_dm1 (2,n,n) alone, without D: d_partial (n_alpha_str, 2n^2) receives <b| E_g |c> restricted to the bra's alpha
 * row Ia (one workgroup per row, one wavefront per generator, the ket row staged in LDS: n_beta_str <= 13312), a
 * second kernel sums it over Ia in ascending order.  d_bra may be d_ket.  No atomics: the same bits every time. */
int nbx_fci_rdm1(nbx_ctx* ctx, int64_t n, int64_t n_alpha_str, int64_t n_beta_str, const int* d_link_a,
                 const int* d_link_bt, const double* d_bra, const double* d_ket, double* d_partial, double* d_dm1);

#ifdef __cplusplus
}
#endif
#endif /* NBX_H */
