// The last stage of huz_scalars_kernel (elementwise.hip) as a device function ONE wavefront of a LATER kernel on the
// same stream runs: the sums over the workgroups' partials, the square roots, the status words and the ready word in
// pinned host memory (nbx_scalars_courier, include/nbx.h).
//
// Why: that stage -- a device-wide fence, a returning arrival atomic, the last workgroup's read of every partial, two
// LDS reductions, system-scope stores -- was 7 of the kernel's 13 us on the SCF's critical path, and the next cycle's
// J/K build needs none of it: only the density and the Dtot' table (DESIGN.md sections 7 and 9).  A deferred scalars
// kernel stops at its partials; the build that follows carries them to the host behind its own first trip to memory
// (jk_m8.hip), or nbx_huz_scalars_flush does in a launch of its own when no build follows.
//
// The sums are those of huz_scalars_kernel's last workgroup, bit for bit: virtual thread `tid` of the `nthreads` of the
// launch that made the partials takes blocks tid, tid + nthreads, ..; nbx_wave_sum_dpp per virtual wave of 64; the
// waves added in ascending order from 0.0; sqrt on entries 2 and 3.  The courier waits on nothing: everything it reads
// was finished by an earlier kernel of the stream.
#pragma once
#include "nbx_common.h"

constexpr int NBX_COURIER_MAX_WAVES = 4;  // launches of 128 and of 256 threads (dim3(16, 8), dim3(32, 8))

// what the host checks before it defers a cycle's scalars or hands a courier to a kernel
inline bool nbx_courier_covers(int nblocks, int nthreads, int nstatus) {
    return nblocks > 0 && (nthreads == 128 || nthreads == 256) && nstatus >= 0 && nstatus <= 64;
}
// the whole description, as a kernel is handed it (the partials are read sixteen bytes at a time)
inline bool nbx_courier_valid(const nbx_scalars_courier& c) {
    return c.d_partial != nullptr && (reinterpret_cast<uintptr_t>(c.d_partial) & 15) == 0 && c.h_out != nullptr &&
           nbx_courier_covers(c.nblocks, c.nthreads, c.nstatus) && (c.nstatus == 0 || c.d_status != nullptr);
}

// (the partials' pointer stays what the caller put there)
inline void nbx_courier_fill(nbx_scalars_courier* c, int nblocks, int nthreads, const int* d_status, int nstatus, double* h_out) {
    c->nblocks = nblocks;
    c->nthreads = nthreads;
    c->d_status = d_status;
    c->nstatus = nstatus;
    c->reserved = 0;
    c->h_out = h_out;
}

// what the carrying wave holds between its request and the stores: the first block of every virtual thread this lane
// stands for, and its status word
struct nbx_courier_regs {
    double p[NBX_COURIER_MAX_WAVES][4];
    int status;
};

// The loads, all in one trip (a caller puts its own loads next to them).  Every lane of the wavefront calls.
__device__ __forceinline__ void nbx_courier_request(const nbx_scalars_courier& c, int lane, nbx_courier_regs& r) {
    const int nwave = c.nthreads >> 6;
#pragma unroll
    for (int v = 0; v < NBX_COURIER_MAX_WAVES; ++v) {
        const int b = v * 64 + lane;
        const bool in = v < nwave && b < c.nblocks;
        const double2* src = reinterpret_cast<const double2*>(c.d_partial + 4 * (int64_t)(in ? b : 0));
        const double2 lo = in ? src[0] : make_double2(0.0, 0.0), hi = in ? src[1] : make_double2(0.0, 0.0);
        r.p[v][0] = lo.x;
        r.p[v][1] = lo.y;
        r.p[v][2] = hi.x;
        r.p[v][3] = hi.y;
    }
    r.status = lane < c.nstatus ? c.d_status[lane] : 0;
}

// The sums and the stores.  Every lane of the wavefront calls (nbx_wave_sum_dpp needs them all).
__device__ __forceinline__ void nbx_courier_deliver(const nbx_scalars_courier& c, int lane, const nbx_courier_regs& r) {
    const int nwave = c.nthreads >> 6;
    double tot[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int v = 0; v < NBX_COURIER_MAX_WAVES; ++v) {
        if (v < nwave) {  // (uniform)
            const int tid = v * 64 + lane;
            double t4[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int o = 0; o < 4; ++o) t4[o] += r.p[v][o];  // (a lane without a block holds 0.0: the sum it starts from)
            for (int b = tid + c.nthreads; b < c.nblocks; b += c.nthreads)  // (none at the sizes a build carries)
#pragma unroll
                for (int o = 0; o < 4; ++o) t4[o] += c.d_partial[(int64_t)b * 4 + o];
#pragma unroll
            for (int o = 0; o < 4; ++o) tot[o] += nbx_wave_sum_dpp(t4[o]);
        }
    }
    double* out = c.h_out;
    if (lane < 4) {
        const double t = lane == 0 ? tot[0] : (lane == 1 ? tot[1] : (lane == 2 ? tot[2] : tot[3]));
        out[lane] = (lane >= 2) ? sqrt(t) : t;
    }
    if (lane < c.nstatus) out[4 + lane] = (double)r.status;
    // the word behind the results says they are all there (huz_scalars_kernel's protocol): every lane's stores are on
    // their way to the host before lane 0 stores it
    __threadfence_system();
    if (lane == 0) __hip_atomic_store(out + 4 + c.nstatus, 1.0, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
