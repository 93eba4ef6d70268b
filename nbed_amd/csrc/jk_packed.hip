// libnbx: the packed J/K entry points (include/nbx.h "J/K contraction, packed form") -- which back-end (jk_packed.h)
// serves a size and as which of its instances, the size queries derived from that, and the zero padding of a size that
// is no instance.
#include "jk_packed.h"
#include "jk_s4_layout.h"

namespace {

struct PackedRoute {
    int kernel;      // NBX_JK_KERNEL_*
    int64_t run_as;  // the instance size: nao, or the next instance with the extra rows and columns zero; 0: none
};

// The one place that knows the precedence of the back-ends and the effect of NBX_JK_M8 / NBX_JK_M4 / NBX_JK_MX (each
// read once per process by its back-end's covers()): a pure function of nao and those switches.
//   jk_mx.hip  takes what is within eight rows of one of its instances (149 .. 400),
//   jk_m8.hip  the sizes whose next multiple of four is one of its instances (97 .. 148), jk_m4.hip likewise behind it,
//   jk_s4.hip  what is within S4_MAX_PAD rows of one of its instances (16 .. 256).
// Quirks, kept as they are (tests/golden/jk_packed_sizes.json records the answers):
//   (a) jk_mx.hip is asked first and is shielded only by jk_m4.hip: with NBX_JK_M4=0 alone 144 .. 148 run on jk_mx.hip's
//       N = 152 instance although jk_m8.hip covers them -- and nbx_jk_packed_fold, which asks jk_m8.hip, says 8 for them;
//   (b) jk_m8.hip / jk_m4.hip are consulted only where jk_s4.hip would serve the size, padded or not;
//   (c) nbx_jk_packed_supported answers 1 / 2 from jk_s4.hip's point of view below jk_mx.hip's range: 1 for 98 although
//       it runs as (M8, 100) -- and nbx_jk_dts_bytes sizes a table in jk_s4.hip's order for 98, which no build reads.
PackedRoute packed_resolve(int64_t nao) {
    if (nao <= 0) return {NBX_JK_KERNEL_NONE, 0};
    const int64_t n4 = (nao + 3) / 4 * 4;
    const bool m4 = nbx_jk_m4_covers(n4);
    if (const int64_t nx = m4 ? 0 : nbx_jk_mx_padded(nao))
        return {nbx_jk_mx_covers_hi(nx) ? NBX_JK_KERNEL_MX_HI : NBX_JK_KERNEL_MX, nx};
    const int64_t ns = s4_padded(nao);
    if (ns == 0) return {NBX_JK_KERNEL_NONE, 0};
    if (nbx_jk_m8_covers(n4)) return {NBX_JK_KERNEL_M8, n4};
    if (m4) return {NBX_JK_KERNEL_M4, n4};
    return {NBX_JK_KERNEL_S4, ns};
}

struct Backend {
    decltype(&nbx_jk_s4_packed_bytes) packed_bytes;
    decltype(&nbx_jk_s4_worksize) worksize;
    decltype(&nbx_jk_s4_pack) pack;
    decltype(&nbx_jk_s4) run;
};
const Backend BACKENDS[] = {  // by NBX_JK_KERNEL_*
    {},
    {nbx_jk_s4_packed_bytes, nbx_jk_s4_worksize, nbx_jk_s4_pack, nbx_jk_s4},
    {nbx_jk_m4_packed_bytes, nbx_jk_m4_worksize, nbx_jk_m4_pack, nbx_jk_m4},
    {nbx_jk_m8_packed_bytes, nbx_jk_m8_worksize, nbx_jk_m8_pack, nbx_jk_m8},
    {nbx_jk_mx_packed_bytes, nbx_jk_mx_worksize, nbx_jk_mx_pack, nbx_jk_mx},
    {nbx_jk_mx_packed_bytes, nbx_jk_mx_worksize, nbx_jk_mx_pack, nbx_jk_mx},  // (MX_HI: nbx_jk_mx* forward)
};

bool is_mx(const PackedRoute& r) { return r.kernel == NBX_JK_KERNEL_MX || r.kernel == NBX_JK_KERNEL_MX_HI; }

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// the padded densities and J/K of a size that is no instance, behind the back-end's workspace
size_t pad_bytes(const PackedRoute& r, int64_t nao, int64_t ndm) {
    return r.run_as != nao ? align256((size_t)((1 + 2 * ndm) * r.run_as * r.run_as) * sizeof(double)) : 0;
}

// (nmat, N, N) -> (nmat, NP, NP) with zero rows/columns appended, and back
__global__ void s4_pad_square_kernel(const double* __restrict__ src, double* __restrict__ dst, int N, int NP, int nmat) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)nmat * NP * NP) return;
    const int b = (int)(i % NP), a = (int)((i / NP) % NP), m = (int)(i / ((int64_t)NP * NP));
    dst[i] = (a < N && b < N) ? src[((int64_t)m * N + a) * N + b] : 0.0;
}
__global__ void s4_crop_square_kernel(const double* __restrict__ src, double* __restrict__ dst, int N, int NP, int nmat) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)nmat * N * N) return;
    const int b = (int)(i % N), a = (int)((i / N) % N), m = (int)(i / ((int64_t)N * N));
    dst[i] = src[((int64_t)m * NP + a) * NP + b];
}

// nao as the run_as x run_as problem whose extra rows and columns are zero (the tiles with p >= nao vanish: never
// stored, never visited): D padded on the way in, J/K cropped on the way out, the Fock assembly its own launch
int run_padded(const PackedRoute& r, nbx_ctx* ctx, int64_t nao, int64_t p0, int64_t p1, const double* d_packed,
               const double* d_dm, int64_t ndm, double* d_jk, void* d_work, const double* d_hv, double* d_fock,
               double* d_vhf) {
    const Backend& be = BACKENDS[r.kernel];
    const int64_t NP = r.run_as, tin = ndm * NP * NP, tout = (1 + ndm) * nao * nao;
    double* dm_pad = reinterpret_cast<double*>(static_cast<char*>(d_work) + be.worksize(NP, p0, p1, ndm));
    double* jk_pad = dm_pad + tin;
    hipLaunchKernelGGL(s4_pad_square_kernel, dim3((unsigned)nbx_cdiv(tin, 256)), dim3(256), 0, ctx->stream, d_dm, dm_pad,
                       (int)nao, (int)NP, (int)ndm);
    NBX_LAUNCH_CHECK();
    const int rc = be.run(ctx, NP, p0, p1, d_packed, dm_pad, ndm, jk_pad, d_work, nullptr, nullptr, nullptr, nullptr);
    if (rc != NBX_OK) return rc;
    hipLaunchKernelGGL(s4_crop_square_kernel, dim3((unsigned)nbx_cdiv(tout, 256)), dim3(256), 0, ctx->stream, jk_pad, d_jk,
                       (int)nao, (int)NP, (int)(1 + ndm));
    NBX_LAUNCH_CHECK();
    if (d_fock != nullptr) return nbx_fock_uhf(ctx, nao, d_hv, 3, nullptr, d_jk, d_fock, d_vhf);
    return NBX_OK;
}

int packed_jk(nbx_ctx* ctx, int64_t nao, int64_t p0, int64_t p1, const double* d_packed, const double* d_dm, int64_t ndm,
              double* d_jk, void* d_work, size_t work_bytes, const double* d_hv, double* d_fock, double* d_vhf,
              const double* d_dts, const nbx_scalars_courier* carry = nullptr) {
    NBX_CHECK_ARG(ctx && d_dm && d_jk);
    NBX_CHECK_ARG(nao > 0 && p0 >= 0 && p1 >= p0 && p1 <= nao);
    NBX_CHECK_ARG(d_packed != nullptr || p0 == p1);
    NBX_CHECK_ARG(ndm == 1 || ndm == 2);
    const PackedRoute r = packed_resolve(nao);
    if (r.kernel == NBX_JK_KERNEL_NONE) {
        nbx_set_error("nbx_jk_packed: N = %lld is not covered (N <= 400 within %d of a size the kernels have an "
                      "instance for)", (long long)nao, S4_MAX_PAD);
        return NBX_E_UNSUPPORTED;
    }
    const size_t need = BACKENDS[r.kernel].worksize(r.run_as, p0, p1, ndm) + pad_bytes(r, nao, ndm);
    if (d_work == nullptr || work_bytes < need) {
        nbx_set_error("nbx_jk_packed: workspace %zu < %zu bytes", work_bytes, need);
        return NBX_E_NOMEM;
    }
    NBX_CHECK_ARG((reinterpret_cast<uintptr_t>(d_packed) & 15) == 0 && (reinterpret_cast<uintptr_t>(d_work) & 15) == 0);
    if (carry != nullptr && carry->d_partial != nullptr) {
        // a deferred cycle's scalars: on their way with jk_m8.hip's kernel, else by a launch of their own ahead of the build
        if (r.kernel == NBX_JK_KERNEL_M8 && r.run_as == nao && p1 > p0)
            return nbx_jk_m8_carry(ctx, nao, p0, p1, d_packed, d_dm, ndm, d_jk, d_work, d_hv, d_fock, d_vhf, d_dts, carry);
        const int rc = nbx_huz_scalars_flush(ctx, carry);
        if (rc != NBX_OK) return rc;
    }
    if (p1 == p0) return nbx_memset(ctx, d_jk, 0, (size_t)((1 + ndm) * nao * nao) * sizeof(double));
    if (r.run_as != nao) return run_padded(r, ctx, nao, p0, p1, d_packed, d_dm, ndm, d_jk, d_work, d_hv, d_fock, d_vhf);
    return BACKENDS[r.kernel].run(ctx, nao, p0, p1, d_packed, d_dm, ndm, d_jk, d_work, d_hv, d_fock, d_vhf, d_dts);
}

}  // namespace

// The one owner of the Dtot' table's layout.  The table is kept in the order of the kernel that runs nao as its own
// instance; jk_mx.hip prepares its table itself (one small launch beside a build of 0.2 .. 2.4 ms) and so does a
// zero-padded run -- but see quirk (c).
size_t nbx_jk_dts_layout(int64_t nao, int* nb4, int* lpt4, int* m4) {
    *nb4 = *lpt4 = *m4 = 0;
    const PackedRoute r = packed_resolve(nao);
    if (r.kernel == NBX_JK_KERNEL_NONE || is_mx(r)) return 0;
    if (r.kernel == NBX_JK_KERNEL_S4 || r.run_as != nao) {  // jk_s4.hip's order: its blocks and loads per thread
        if (!nbx_jk_s4_covers(nao)) return 0;
        *nb4 = s4_nb(nao);
        *lpt4 = s4_lpt(nao);
        return (size_t)(*nb4 * *nb4 * *lpt4 * 128) * sizeof(double);
    }
    // jk_m4.hip's staging order, for jk_m8.hip with its own chunk boundaries when it has four chunks
    const bool m8 = r.kernel == NBX_JK_KERNEL_M8;
    int wl[4];
    (m8 ? nbx_jk_m8_weight_layout : nbx_jk_m4_weight_layout)(nao, wl);
    if (wl[3] == 0) return 0;
    *nb4 = wl[0];
    *lpt4 = wl[1];
    *m4 = (wl[2] << 8) | wl[3];
    return m8 ? nbx_jk_m8_weights_bytes(nao) : nbx_jk_m4_weights_bytes(nao);
}

bool nbx_jk_packed_carries(int64_t nao) {
    const PackedRoute r = packed_resolve(nao);
    return r.kernel == NBX_JK_KERNEL_M8 && r.run_as == nao;
}

int nbx_jk_packed_fock_carry(nbx_ctx* ctx, int64_t nao, const double* d_packed, const double* d_dm, const double* d_hv,
                             double* d_jk, double* d_fock, double* d_vhf, void* d_work, size_t work_bytes,
                             const double* d_dts, const nbx_scalars_courier* carry) {
    NBX_CHECK_ARG(d_hv && d_fock);
    return packed_jk(ctx, nao, 0, nao, d_packed, d_dm, 2, d_jk, d_work, work_bytes, d_hv, d_fock, d_vhf, d_dts, carry);
}

extern "C" {

// 1: a kernel instance serves N; 2: served as the next covered size with zero rows/columns; 0: no -- quirk (c)
int nbx_jk_packed_supported(int64_t nao) {
    const PackedRoute r = packed_resolve(nao);
    if (r.kernel == NBX_JK_KERNEL_NONE) return 0;
    return (is_mx(r) ? r.run_as == nao : nbx_jk_s4_covers(nao)) ? 1 : 2;
}

int nbx_jk_packed_fold(int64_t nao) {
    if (packed_resolve(nao).kernel == NBX_JK_KERNEL_NONE) return 0;
    return nbx_jk_m8_covers((nao + 3) / 4 * 4) ? 8 : 4;  // (not "the route is M8": quirk (a))
}

// Test support (include/nbx.h): the resolver's answer
int nbx_jk_packed_route(int64_t nao, int* kernel, int* run_as) {
    if (kernel == nullptr || run_as == nullptr) return NBX_E_INVALID;
    const PackedRoute r = packed_resolve(nao);
    *kernel = r.kernel;
    *run_as = (int)r.run_as;
    return NBX_OK;
}

size_t nbx_eri_packed_bytes(int64_t nao, int64_t p0, int64_t p1) {
    if (p0 < 0 || p1 < p0 || p1 > nao) return 0;
    const PackedRoute r = packed_resolve(nao);
    return r.kernel == NBX_JK_KERNEL_NONE ? 0 : BACKENDS[r.kernel].packed_bytes(r.run_as, p0, p1);
}

// (of a zero-padded size: the tiles (p, q) with p < nao of the padded tensor -- the others are zero)
int nbx_eri_pack(nbx_ctx* ctx, int64_t nao, int64_t p0, int64_t p1, const double* d_eri, double* d_packed) {
    NBX_CHECK_ARG(ctx);
    NBX_CHECK_ARG(nao > 0 && p0 >= 0 && p1 >= p0 && p1 <= nao);
    const PackedRoute r = packed_resolve(nao);
    if (r.kernel == NBX_JK_KERNEL_NONE) {
        nbx_set_error("nbx_eri_pack: N = %lld is not covered by the packed J/K kernel", (long long)nao);
        return NBX_E_UNSUPPORTED;
    }
    if (p0 == p1) return NBX_OK;
    NBX_CHECK_ARG(d_eri && d_packed);
    return BACKENDS[r.kernel].pack(ctx, r.run_as, nao, p0, p1, d_eri, d_packed);
}

size_t nbx_jk_packed_worksize(int64_t nao, int64_t p0, int64_t p1, int64_t ndm) {
    if (p0 < 0 || p1 < p0 || p1 > nao || ndm <= 0) return 0;
    const PackedRoute r = packed_resolve(nao);
    if (r.kernel == NBX_JK_KERNEL_NONE) return 0;
    return BACKENDS[r.kernel].worksize(r.run_as, p0, p1, ndm) + pad_bytes(r, nao, ndm);
}

size_t nbx_jk_dts_bytes(int64_t nao) {
    int nb4, lpt4, m4;
    return nbx_jk_dts_layout(nao, &nb4, &lpt4, &m4);
}

int nbx_jk_dts_init(nbx_ctx* ctx, int64_t nao, double* d_dts) {
    NBX_CHECK_ARG(ctx && d_dts && nbx_jk_dts_bytes(nao) > 0);
    return nbx_memset(ctx, d_dts, 0, nbx_jk_dts_bytes(nao));
}

int nbx_jk_packed(nbx_ctx* ctx, int64_t nao, int64_t p0, int64_t p1, const double* d_packed, const double* d_dm,
                  int64_t ndm, double* d_jk, void* d_work, size_t work_bytes) {
    return packed_jk(ctx, nao, p0, p1, d_packed, d_dm, ndm, d_jk, d_work, work_bytes, nullptr, nullptr, nullptr, nullptr);
}

int nbx_jk_packed_fock(nbx_ctx* ctx, int64_t nao, const double* d_packed, const double* d_dm, const double* d_hv,
                       double* d_jk, double* d_fock, double* d_vhf, void* d_work, size_t work_bytes, const double* d_dts) {
    NBX_CHECK_ARG(d_hv && d_fock);
    return packed_jk(ctx, nao, 0, nao, d_packed, d_dm, 2, d_jk, d_work, work_bytes, d_hv, d_fock, d_vhf, d_dts);
}

}  // extern "C"
