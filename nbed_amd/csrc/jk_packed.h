// The back-ends of the packed J/K contraction and what its dispatcher (jk_packed.hip: nbx_eri_pack, nbx_jk_packed,
// nbx_jk_packed_fock and their size queries) shares with the rest of the library.
//
// A back-end is a file with kernel instances for a set of sizes N; it exports five functions:
//   covers(N)                         : N is one of its instances (and its environment switch, if it has one, is not 0)
//   packed_bytes(N, p0, p1)           : bytes of the packed tiles of rows [p0, p1)
//   worksize(N, p0, p1, ndm)          : bytes of workspace of a run
//   pack(ctx, N, nsrc, p0, p1, ...)   : rows [p0, p1) of a dense tensor of size nsrc <= N, the rows and columns beyond
//                                       nsrc zero, into instance N's tile format
//   run(ctx, N, p0, p1, ..., d_dts)   : J/K of the slab, with the Fock epilogue when d_fock is given; d_dts: NULL, or the
//                                       Dtot' table of d_dm in this back-end's order (jk_mx.hip makes its own: ignored)
// The dispatcher alone decides which of them serves a size (packed_resolve); no back-end calls another.
#pragma once
#include "nbx_common.h"

#define NBX_JK_BACKEND(covers, packed_bytes, worksize, pack, run)                                                        \
    bool covers(int64_t N);                                                                                              \
    size_t packed_bytes(int64_t N, int64_t p0, int64_t p1);                                                              \
    size_t worksize(int64_t N, int64_t p0, int64_t p1, int64_t ndm);                                                     \
    int pack(nbx_ctx* ctx, int64_t N, int64_t nsrc, int64_t p0, int64_t p1, const double* d_eri, double* d_packed);      \
    int run(nbx_ctx* ctx, int64_t N, int64_t p0, int64_t p1, const double* d_packed, const double* d_dm, int64_t ndm,    \
            double* d_jk, void* d_work, const double* d_hv, double* d_fock, double* d_vhf, const double* d_dts);
// jk_s4.hip: 4-fold tiles walked on the vector ALU, even N = 24 .. 256
NBX_JK_BACKEND(nbx_jk_s4_covers, nbx_jk_s4_packed_bytes, nbx_jk_s4_worksize, nbx_jk_s4_pack, nbx_jk_s4)
// jk_m4.hip: 4-fold 4 x 4 blocks on the matrix cores, N = 100 .. 148 in steps of four, unless NBX_JK_M4=0
NBX_JK_BACKEND(nbx_jk_m4_covers, nbx_jk_m4_packed_bytes, nbx_jk_m4_worksize, nbx_jk_m4_pack, nbx_jk_m4)
// jk_m8.hip: the 8-fold form of the same sizes, unless NBX_JK_M8=0
NBX_JK_BACKEND(nbx_jk_m8_covers, nbx_jk_m8_packed_bytes, nbx_jk_m8_worksize, nbx_jk_m8_pack, nbx_jk_m8)
// jk_mx.hip: the walk of jk_m4.hip with a tile in more chunks, N = 152 .. 400, unless NBX_JK_MX=0; it forwards the sizes
// above 256 to the instances of its second translation unit, jk_mx_hi.hip, itself
NBX_JK_BACKEND(nbx_jk_mx_covers, nbx_jk_mx_packed_bytes, nbx_jk_mx_worksize, nbx_jk_mx_pack, nbx_jk_mx)
NBX_JK_BACKEND(nbx_jk_mx_covers_hi, nbx_jk_mx_packed_bytes_hi, nbx_jk_mx_worksize_hi, nbx_jk_mx_pack_hi, nbx_jk_mx_hi)
#undef NBX_JK_BACKEND
// jk_m8.hip's run with one more argument: the scalars of a deferred SCF cycle (include/nbx.h nbx_scalars_courier) that its
// kernel takes to the host in its prologue; NULL: nbx_jk_m8.  The other back-ends carry nothing: a cycle whose next
// build would run on them is not deferred (nbx_jk_packed_carries), and what arrives anyway is flushed ahead of the build.
int nbx_jk_m8_carry(nbx_ctx* ctx, int64_t N, int64_t p0, int64_t p1, const double* d_packed, const double* d_dm, int64_t ndm,
                    double* d_jk, void* d_work, const double* d_hv, double* d_fock, double* d_vhf, const double* d_dts,
                    const nbx_scalars_courier* carry);
// jk_packed.hip: the whole-tensor build of size nao runs on a kernel that carries (jk_m8.hip, nao its own instance);
// nbx_jk_packed_fock with the courier
bool nbx_jk_packed_carries(int64_t nao);
int nbx_jk_packed_fock_carry(nbx_ctx* ctx, int64_t nao, const double* d_packed, const double* d_dm, const double* d_hv,
                             double* d_jk, double* d_fock, double* d_vhf, void* d_work, size_t work_bytes,
                             const double* d_dts, const nbx_scalars_courier* carry);
// the jk_mx.hip instance N runs as: N itself or the next one, at most eight zero rows and columns more; 0: none
int64_t nbx_jk_mx_padded(int64_t N);

// The Dtot' table a density's judge (huz_scalars_kernel) can leave for the next build in jk_m4.hip's / jk_m8.hip's
// order: its bytes and the first block rows of chunks 1 .. 3 and the slots per chunk (all zero: the instance has more
// than four chunks and makes its table itself)
size_t nbx_jk_m4_weights_bytes(int64_t N);
void nbx_jk_m4_weight_layout(int64_t N, int out[4]);
size_t nbx_jk_m8_weights_bytes(int64_t N);
void nbx_jk_m8_weight_layout(int64_t N, int out[4]);

// jk_packed.hip: the bytes of the Dtot' table of size nao (nbx_jk_dts_bytes; 0: there is none) and the launch parameters
// (s4_nb_, s4_lpt_, dts_m4) with which huz_scalars_kernel writes it in the order of the kernel that will read it
size_t nbx_jk_dts_layout(int64_t nao, int* nb4, int* lpt4, int* m4);
