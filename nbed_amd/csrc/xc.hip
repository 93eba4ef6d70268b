// libnbx: the exchange-correlation quadrature of the embedding-potential producer -- what the
// reference gets from PySCF's numint + libxc behind `dft.UKS.get_veff` (nbed/driver.py:155-191 global Kohn-Sham,
// :315-431 `_subsystem_dft`, :845-852 the embedding potential, :1138-1231 DFT-in-DFT).  One evaluation of
// (E_xc, v_xc) for a two-spin density matrix is three kernels over the stored AO values ao (G, nao) and gradients
// dao (3, G, nao) of the molecular grid (grid.hip makes them).  Each kernel has a tau form for the meta-GGAs (TPSS,
// TPSSh), which carries the kinetic-energy density tau_x = 1/2 sum_i |grad psi_i|^2 through the same body: a template
// parameter, so the plain instantiations hold none of it.
//
//   xc_rho_kernel      c = ao D on the matrix cores (v_mfma_f64_16x16x4_f64), tile by tile, BOTH spins from one pass
//                      over ao; the tile never leaves the registers: rho = sum_m c ao and grad rho = 2 sum_m c dao
//                      are reduced in the epilogue (dao is read exactly once)                      -- MFMA bound
//                      TAU: three more products per tile, dao_a D against dao_a: tau = 1/2 sum_a sum_m (dao_a D) dao_a
//   xc_functional_kernel  one thread per grid point: energy density and its first derivatives with respect to
//                      (rho_a, rho_b, sigma_aa, sigma_ab, sigma_bb) written out analytically (Slater, Becke 88,
//                      VWN-RPA / VWN5, LYP in Miehlich's form: libxc's B3LYP = 0.08 S + 0.72 B88 + 0.19 VWN_RPA +
//                      0.81 LYP + 0.2 HF, B3LYP5 with VWN5, BLYP; PBE exchange, Perdew-Wang 1992 and PBE
//                      correlation: PBE, PBEH), one instantiation per functional, quadrature weights folded in, E_xc
//                      and the electron count reduced in a fixed order                              -- ALU (exp, log, cbrt)
//                      the TPSS codes read tau and write the derivative with respect to it as well
//   xc_vmat_kernel     v[m][n] = sum_g ao[g][m] half[g][n],  half = v_rho / 2 ao + (2 v_ss grad rho_s + v_ab grad
//                      rho_o) . dao, with `half` built ON THE FLY as the B operand (it never exists in memory), split
//                      over chunks of grid points; xc_vmat_reduce_kernel adds the chunks in a fixed order and
//                      symmetrises (v + v^T)                                                        -- MFMA bound
//                      TAU: + sum_a dao_a[g][m] (v_tau / 4 dao_a)[g][n], three more operands per step of grid points
#include "nbx_common.h"

namespace {

typedef double xc_v4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------------ density pass
// A workgroup = 4 waves = 64 grid points; wave w owns points g0 + 16 w .. + 16.  For every 16-column tile of
// c = ao D: the (nao x 16) slab of D (both spins) goes to LDS once per workgroup; A fragments ao[g][k] are kept
// in registers across the column tiles when nao <= 4 AREG.  C layout of the 16x16x4 product: acc[r] of lane
// (fk = lane >> 4, fr = lane & 15) is element (row fk + 4 r, column fr).
// TAU (`tau` is written by no other instantiation; null there): after c = ao D the slab of D that is already in LDS is multiplied by
// the fragments of dao_x, dao_y and dao_z in turn (streamed: 3 x 40 doubles would not fit beside the ao fragments), and
// each product is reduced against the dao_a values the epilogue of rho has just read.  The passes are sequential inside
// the tile loop, two accumulators live at a time; rho and grad rho are the plain kernel's bit for bit (same fragments,
// same order, same epilogue).                                                                -- MFMA bound, 4 x plain
template <int AREG, bool TAU>
__global__ __launch_bounds__(256) void xc_rho_kernel(int64_t npts, int nao, const double* __restrict__ ao,
                                                     const double* __restrict__ dao, const double* __restrict__ dm,
                                                     double* __restrict__ rho, double* __restrict__ grad,
                                                     double* __restrict__ tau) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int KP = (nao + 3) & ~3, NT = (nao + 15) >> 4, NK = KP >> 2;
    double* ds0 = smem;             // [KP][16]  D_alpha[:, tile]
    double* ds1 = smem + KP * 16;   // [KP][16]  D_beta
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fr = lane & 15, fk = lane >> 4;
    const int64_t gw = (int64_t)blockIdx.x * 64 + wave * 16;
    const int64_t plane = npts * (int64_t)nao, n2 = (int64_t)nao * nao;
    const int64_t ga = gw + fr;  // the A-fragment row of this lane
    const bool a_ok = ga < npts;
    const double* arow = ao + (a_ok ? ga : 0) * nao;
    double afr[AREG > 0 ? AREG : 1];
    if (AREG > 0) {
#pragma unroll
        for (int j = 0; j < AREG; ++j) {
            const int k = 4 * j + fk;
            afr[j] = (a_ok && k < nao) ? arow[k] : 0.0;
        }
    }
    double pr[2][4], px[2][4], py[2][4], pz[2][4], pt[2][4];  // (pt: TAU only)
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int r = 0; r < 4; ++r) pr[x][r] = px[x][r] = py[x][r] = pz[x][r] = pt[x][r] = 0.0;

    for (int ct = 0; ct < NT; ++ct) {
        __syncthreads();  // the previous tile's fragments have been read
        for (int e = threadIdx.x; e < KP * 16; e += 256) {
            const int k = e >> 4, c = 16 * ct + (e & 15);
            const bool in = k < nao && c < nao;
            ds0[e] = in ? dm[(int64_t)k * nao + c] : 0.0;
            ds1[e] = in ? dm[n2 + (int64_t)k * nao + c] : 0.0;
        }
        __syncthreads();
        xc_v4 acc0 = (xc_v4){0.0, 0.0, 0.0, 0.0}, acc1 = (xc_v4){0.0, 0.0, 0.0, 0.0};
        if (AREG > 0) {
#pragma unroll
            for (int j = 0; j < AREG; ++j) {
                if (j < NK) {
                    const int k = 4 * j + fk;
                    acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(afr[j], ds0[k * 16 + fr], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(afr[j], ds1[k * 16 + fr], acc1, 0, 0, 0);
                }
            }
        } else {
            for (int j = 0; j < NK; ++j) {
                const int k = 4 * j + fk;
                const double a = (a_ok && k < nao) ? arow[k] : 0.0;
                acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, ds0[k * 16 + fr], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, ds1[k * 16 + fr], acc1, 0, 0, 0);
            }
        }
        // epilogue: this tile of c against the same tile of ao / dao; TAU: the dao values stay for the tau products
        const int m = 16 * ct + fr;
        double dv[3][4];
        if constexpr (TAU) {
#pragma unroll
            for (int r = 0; r < 4; ++r) dv[0][r] = dv[1][r] = dv[2][r] = 0.0;
        }
        if (m < nao) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t g = gw + fk + 4 * r;
                if (g < npts) {
                    const int64_t off = g * nao + m;
                    const double v0 = ao[off], vx = dao[off], vy = dao[plane + off], vz = dao[2 * plane + off];
                    pr[0][r] = fma(acc0[r], v0, pr[0][r]);
                    px[0][r] = fma(acc0[r], vx, px[0][r]);
                    py[0][r] = fma(acc0[r], vy, py[0][r]);
                    pz[0][r] = fma(acc0[r], vz, pz[0][r]);
                    pr[1][r] = fma(acc1[r], v0, pr[1][r]);
                    px[1][r] = fma(acc1[r], vx, px[1][r]);
                    py[1][r] = fma(acc1[r], vy, py[1][r]);
                    pz[1][r] = fma(acc1[r], vz, pz[1][r]);
                    if constexpr (TAU) dv[0][r] = vx, dv[1][r] = vy, dv[2][r] = vz;
                }
            }
        }
        if constexpr (TAU) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double* drow = dao + a * plane + (a_ok ? ga : 0) * nao;
                xc_v4 t0 = (xc_v4){0.0, 0.0, 0.0, 0.0}, t1 = (xc_v4){0.0, 0.0, 0.0, 0.0};
                for (int j = 0; j < NK; ++j) {
                    const int k = 4 * j + fk;
                    const double d = (a_ok && k < nao) ? drow[k] : 0.0;
                    t0 = __builtin_amdgcn_mfma_f64_16x16x4f64(d, ds0[k * 16 + fr], t0, 0, 0, 0);
                    t1 = __builtin_amdgcn_mfma_f64_16x16x4f64(d, ds1[k * 16 + fr], t1, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {  // (dv = 0 outside the arrays)
                    pt[0][r] = fma(t0[r], dv[a][r], pt[0][r]);
                    pt[1][r] = fma(t1[r], dv[a][r], pt[1][r]);
                }
            }
        }
    }
    // sum over the 16 lanes (columns) that share the rows fk + 4 r: xor shuffles stay inside the 16-lane group
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double a = pr[x][r], b = px[x][r], c = py[x][r], d = pz[x][r], t = pt[x][r];
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) {
                a += __shfl_xor(a, o, 64);
                b += __shfl_xor(b, o, 64);
                c += __shfl_xor(c, o, 64);
                d += __shfl_xor(d, o, 64);
                if constexpr (TAU) t += __shfl_xor(t, o, 64);
            }
            const int64_t g = gw + fk + 4 * r;
            if (fr == 0 && g < npts) {
                rho[x * npts + g] = a;
                grad[(3 * x + 0) * npts + g] = 2.0 * b;
                grad[(3 * x + 1) * npts + g] = 2.0 * c;
                grad[(3 * x + 2) * npts + g] = 2.0 * d;
                if constexpr (TAU) tau[x * npts + g] = 0.5 * t;
            }
        }
}

// ------------------------------------------------------------------------------------------------ functionals
// Each piece returns the energy per volume and adds its first derivatives, scaled by `s`, to the five outputs.
struct XcDer {
    double e, va, vb, vaa, vab, vbb;
};

__device__ __forceinline__ void xc_slater(double s, double ra, double rb, XcDer& o) {
    const double cx = 0.9305257363491002;  // (3/2) (3 / (4 pi))^(1/3)
    const double ca = cbrt(ra), cb = cbrt(rb);
    o.e += s * (-cx * (ca * ra + cb * rb));
    o.va += s * (-(4.0 / 3.0) * cx * ca);
    o.vb += s * (-(4.0 / 3.0) * cx * cb);
}

// Becke's 1988 gradient correction for one spin channel: e = -beta rho^(4/3) g(x), g = x^2 / (1 + 6 beta x asinh x),
// x = sqrt(sigma) / rho^(4/3);  de/drho = -(4/3) beta rho^(1/3) (g - x g'),  de/dsigma = -beta (g'/x) / (2 rho^(4/3))
__device__ __forceinline__ void xc_b88(double s, double r, double sg, double& e, double& vr, double& vs) {
    const double beta = 0.0042;
    const double r13 = cbrt(r), r43 = r13 * r;
    const double x = sqrt(sg) / r43;
    const double ash = asinh(x);
    const double den = fma(6.0 * beta * x, ash, 1.0);
    const double g = x * x / den;
    const double gpx = (2.0 * den - 6.0 * beta * x * (ash + x / sqrt(fma(x, x, 1.0)))) / (den * den);
    e += s * (-beta * r43 * g);
    vr += s * (-(4.0 / 3.0) * beta * r13 * (g - x * x * gpx));
    vs += s * (-beta * gpx / (2.0 * r43));
}

// The attenuation factor of Iikura, Tsuneda, Yanai and Hirao (J. Chem. Phys. 115, 3540 (2001)),
//   F(a) = 1 - (8/3) a [sqrt(pi) erf(1 / (2a)) + 2a (b - c)],  b = exp(-1 / (4 a^2)) - 1,  c = 2 a^2 b + 1/2,
// and P = F + a F' / 2, the combination both derivatives of the short-range exchange need:
//   a F' = -(8/3) a [sqrt(pi) erf(1 / (2a)) + 2 a b - 16 a^3 b - 4 a].
// The bracket tends to 3/8 while F falls like 1 / (36 a^2): in float64 the closed form loses 36 a^4 ulp.  With
// t = 1 / (4 a^2) every term is a power series in t and the sum is F = sum_{m >= 1} c_m t^m,
//   c_m = -(8/3) (-1)^m [1 / (m! (2m + 1)) - 1 / (2 (m + 1)!) - 1 / (4 (m + 2)!)]   (c_1 = 1/9: F -> 1 / (36 a^2)),
// a F' = -2 sum m c_m t^m, so P = sum (1 - m) c_m t^m starts at t^2: formed as F + a F' / 2 it would lose 27 a^2 ulp more,
// summed term by term it loses none.  Sixteen terms from a = 1/2 on (t <= 1), the closed form below: measured against
// 80 digits the series is good to 3e-16 relative from the switch on and the closed form to 1.3e-15 below it (DESIGN.md
// section 17; at a = 0.4 the series is at 1e-13, at a = 0.7 the closed form at 1.2e-14).  a < 1e-60 (omega = 0):
// F = 1 - (8/3) sqrt(pi) a, where 1 / a^4 would overflow in a derivative.
__device__ __forceinline__ void xc_ityh(double a, double& f, double& p) {
    constexpr double C[16] = {1.0 / 9.0, -1.0 / 60.0, 1.0 / 420.0, -1.0 / 3240.0, 1.0 / 27720.0, -1.0 / 262080.0, 1.0 / 2721600.0,
                              -1.0 / 30844800.0, 1.0 / 379209600.0, -1.0 / 5029516800.0, 1.0 / 71610739200.0,
                              -1.0 / 1089728640000.0, 1.0 / 17653603968000.0, -1.0 / 303380453376000.0,
                              1.0 / 5513155135488000.0, -1.0 / 105639166144512000.0};
    const double sqrt_pi = 1.7724538509055159;
    if (a >= 0.5) {
        const double t = 0.25 / (a * a);
        double sf = C[15], sp = 15.0 * C[15];
#pragma unroll
        for (int m = 15; m >= 1; --m) {
            sf = fma(sf, t, C[m - 1]);
            sp = fma(sp, t, (m - 1) * C[m - 1]);
        }
        f = t * sf;
        p = -t * sp;
    } else if (a < 1.0e-60) {
        f = 1.0 - (8.0 / 3.0) * sqrt_pi * a;
        p = 1.0 - 4.0 * sqrt_pi * a;
    } else {
        const double b = expm1(-0.25 / (a * a)), er = sqrt_pi * erf(0.5 / a);
        const double c = fma(2.0 * a * a, b, 0.5);
        f = 1.0 - (8.0 / 3.0) * a * (er + 2.0 * a * (b - c));
        p = f - (4.0 / 3.0) * a * (er + 2.0 * a * b - 16.0 * a * a * a * b - 4.0 * a);
    }
}

// Short-range B88 exchange of one spin channel in the ITYH scheme: with the whole B88 exchange e = -rho^(4/3) G(x),
// G = cx + beta g(x) (Slater + Becke's correction, xc_b88's g), written as -1/2 rho^(4/3) K, K = 2 G, the local Fermi
// wave vector is k = sqrt(9 pi / K) rho^(1/3) ((6 pi^2 rho)^(1/3) for G = cx), a = omega / (2 k) and e_sr = e F(a).
// With da/drho = -a (1 + 2 x G'/G) / (3 rho), da/dsigma = a G' / (2 G) dx/dsigma and P = F + a F' / 2:
//   de/drho   = rho^(1/3) [G (-2 F + (2/3) P) + (4/3) x G' P],   x G' = beta x^2 (g'/x)
//   de/dsigma = -beta (g'/x) P / (2 rho^(4/3))
__device__ __forceinline__ void xc_b88_sr(double s, double omega, double r, double sg, double& e, double& vr, double& vs) {
    const double beta = 0.0042, cx = 0.9305257363491002;
    const double r13 = cbrt(r), r43 = r13 * r;
    const double x = sqrt(sg) / r43;
    const double ash = asinh(x);
    const double den = fma(6.0 * beta * x, ash, 1.0);
    const double g = x * x / den;
    const double gpx = (2.0 * den - 6.0 * beta * x * (ash + x / sqrt(fma(x, x, 1.0)))) / (den * den);
    const double G = fma(beta, g, cx), xG1 = beta * x * x * gpx;
    const double a = omega * sqrt(2.0 * G) / (10.634723105433095 * r13);  // 6 sqrt(pi)
    double f, p;
    xc_ityh(a, f, p);
    e += s * (-r43 * G * f);
    vr += s * r13 * (G * ((2.0 / 3.0) * p - 2.0 * f) + (4.0 / 3.0) * xG1 * p);
    vs += s * (-beta * gpx * p / (2.0 * r43));
}

// VWN's interpolation formula eps(x), x = sqrt(rs), and d eps / dx
__device__ __forceinline__ void xc_vwn_fit(double x, double a, double x0, double b, double c, double& e, double& de) {
    const double q = sqrt(4.0 * c - b * b);
    const double X = fma(x, x + b, c), X0 = fma(x0, x0 + b, c);
    const double tb = 2.0 * x + b;
    const double at = atan(q / tb);
    const double den = fma(tb, tb, q * q);
    const double xm = x - x0;
    e = a * (log(x * x / X) + 2.0 * b / q * at - b * x0 / X0 * (log(xm * xm / X) + 2.0 * (b + 2.0 * x0) / q * at));
    de = a * (2.0 / x - tb / X - 4.0 * b / den - b * x0 / X0 * (2.0 / xm - tb / X - 4.0 * (b + 2.0 * x0) / den));
}

// VWN correlation: RPA = false the fit to the Ceperley-Alder data with the paper's spin interpolation (libxc
// LDA_C_VWN: PySCF's "vwn"), RPA = true the fit to the RPA data (LDA_C_VWN_RPA: the one inside B3LYP)
template <bool RPA>
__device__ __forceinline__ void xc_vwn(double s, double ra, double rb, XcDer& o) {
    const double rho = ra + rb;
    const double zeta = (ra - rb) / rho;
    const double x = sqrt(cbrt(0.238732414637843 / rho));  // sqrt(rs), rs = (3 / (4 pi rho))^(1/3)
    const double c43 = 0.5198420997897464;                   // 2^(4/3) - 2
    const double up = 2.0 * ra / rho, dn = 2.0 * rb / rho;  // 1 +- zeta, never by subtraction: zeta -> +-1 when a spin is empty
    const double cp = cbrt(up), cm = cbrt(dn);
    const double fz = (cp * up + cm * dn - 2.0) / c43;
    const double dfz = (4.0 / 3.0) * (cp - cm) / c43;
    double ep, dep, ef, def, eps, dx, dz;
    if (RPA) {
        xc_vwn_fit(x, 0.0310907, -0.409286, 13.0720, 42.7198, ep, dep);
        xc_vwn_fit(x, 0.01554535, -0.743294, 20.1231, 101.578, ef, def);
        eps = fma(fz, ef - ep, ep);
        dx = fma(fz, def - dep, dep);
        dz = dfz * (ef - ep);
    } else {
        double al, dal;
        xc_vwn_fit(x, 0.0310907, -0.10498, 3.72744, 12.9352, ep, dep);
        xc_vwn_fit(x, 0.01554535, -0.32500, 7.06042, 18.0578, ef, def);
        xc_vwn_fit(x, -0.01688686394038963, -0.0047584, 1.13107, 13.0045, al, dal);  // -1 / (6 pi^2): spin stiffness
        const double fpp0 = 1.7099209341613653;  // 4 / (9 (2^(1/3) - 1))
        const double z3 = zeta * zeta * zeta, z4 = z3 * zeta;
        const double omz4 = up * dn * fma(zeta, zeta, 1.0);  // 1 - zeta^4 as a product of its factors
        eps = ep + al * fz / fpp0 * omz4 + (ef - ep) * fz * z4;
        dx = dep + dal * fz / fpp0 * omz4 + (def - dep) * fz * z4;
        dz = al / fpp0 * (dfz * omz4 - 4.0 * fz * z3) + (ef - ep) * (dfz * z4 + 4.0 * fz * z3);
    }
    // e = rho eps(rs, zeta):  d/d rho_s = eps - (rs / 3) d eps / d rs  +-  (1 -+ zeta) d eps / d zeta,  d/d rs = (d/dx) / (2 x)
    const double common = eps - (x / 6.0) * dx;
    o.e += s * rho * eps;
    o.va += s * (common + dn * dz);
    o.vb += s * (common - up * dz);
}

// Lee-Yang-Parr in the gradient-only form of Miehlich, Savin, Stoll and Preuss (CPL 157, 200 (1989)):
//   e = -4 a rho_a rho_b / (rho (1 + d r)) - a b omega [rho_a rho_b P + Q],   r = rho^(-1/3),
//   omega = exp(-c r) / (1 + d r) rho^(-11/3),  delta = c r + d r / (1 + d r),
//   d omega / d rho = omega (delta - 11) / (3 rho),  d delta / d rho = -(delta - (d r / (1 + d r))^2) / (3 rho)
__device__ __forceinline__ void xc_lyp(double s, double ra, double rb, double saa, double sab, double sbb, XcDer& o) {
    const double a = 0.04918, b = 0.132, c = 0.2533, d = 0.349;
    const double rho = ra + rb, rho2 = rho * rho;
    const double r = 1.0 / cbrt(rho);
    const double den = fma(d, r, 1.0);
    const double r113 = r * r / (rho2 * rho);  // rho^(-11/3) = rho^(-2/3) / rho^3
    const double omega = exp(-c * r) / den * r113;
    const double dr = d * r / den;
    const double delta = c * r + dr;
    const double k1 = 36.46239897876477;  // 2^(11/3) (3/10) (3 pi^2)^(2/3)
    const double st = saa + 2.0 * sab + sbb;
    const double ca = cbrt(ra), cb = cbrt(rb);
    const double ra53 = ca * ca * ra, rb53 = cb * cb * rb;  // rho^(5/3)
    const double mix = (ra * saa + rb * sbb) / rho;
    const double P = k1 * (ra53 * ra + rb53 * rb) + (47.0 / 18.0 - 7.0 * delta / 18.0) * st - (2.5 - delta / 18.0) * (saa + sbb) -
                     (delta - 11.0) / 9.0 * mix;
    // the paper's -2/3 rho^2 st + (2/3 rho^2 - ra^2) sbb + (2/3 rho^2 - rb^2) saa with the rho^2 sigma_ss terms, which
    // cancel, taken out (they swamp what is left when one spin is nearly empty)
    const double Q = -4.0 / 3.0 * rho2 * sab - ra * ra * sbb - rb * rb * saa;
    const double B = ra * rb * P + Q;
    const double ab = a * b;
    o.e += s * (-4.0 * a * ra * rb / (rho * den) - ab * omega * B);
    const double dom = omega * (delta - 11.0) / (3.0 * rho);
    const double ddel = -(delta - dr * dr) / (3.0 * rho);
    const double dPdd = -7.0 * st / 18.0 + (saa + sbb) / 18.0 - mix / 9.0;
    const double t1c = d * r / (3.0 * rho * den * den);
    {   // d / d rho_a
        const double dt1 = -4.0 * a * (rb / (rho * den) - ra * rb / (rho2 * den) + ra * rb / rho * t1c);
        const double dP = k1 * (8.0 / 3.0) * ra53 + ddel * dPdd - (delta - 11.0) / 9.0 * (saa - mix) / rho;
        const double dQ = -8.0 / 3.0 * rho * sab - 2.0 * ra * sbb;
        o.va += s * (dt1 - ab * (dom * B + omega * (rb * P + ra * rb * dP + dQ)));
    }
    {   // d / d rho_b
        const double dt1 = -4.0 * a * (ra / (rho * den) - ra * rb / (rho2 * den) + ra * rb / rho * t1c);
        const double dP = k1 * (8.0 / 3.0) * rb53 + ddel * dPdd - (delta - 11.0) / 9.0 * (sbb - mix) / rho;
        const double dQ = -8.0 / 3.0 * rho * sab - 2.0 * rb * saa;
        o.vb += s * (dt1 - ab * (dom * B + omega * (ra * P + ra * rb * dP + dQ)));
    }
    const double abw = -ab * omega;
    o.vaa += s * abw * (ra * rb * (1.0 / 9.0 - delta / 3.0 - (delta - 11.0) / 9.0 * ra / rho) - rb * rb);
    o.vbb += s * abw * (ra * rb * (1.0 / 9.0 - delta / 3.0 - (delta - 11.0) / 9.0 * rb / rho) - ra * ra);
    o.vab += s * abw * (ra * rb * 2.0 * (47.0 / 18.0 - 7.0 * delta / 18.0) - 4.0 / 3.0 * rho2);
}

// Perdew-Burke-Ernzerhof exchange for one spin channel (libxc GGA_X_PBE, spin-scaled): e = -cx rho^(4/3) F(p),
// p = s^2 = sigma / (4 (6 pi^2)^(2/3) rho^(8/3)),  F = 1 + kappa - kappa / (1 + mu p / kappa) = 1 + kappa mu p / (kappa + mu p),
// F' = kappa^2 mu / (kappa + mu p)^2;  de/drho = -(4/3) cx rho^(1/3) (F - 2 p F'),  de/dsigma = -cx F' / (4 (6 pi^2)^(2/3) rho^(4/3))
__device__ __forceinline__ void xc_pbe_x(double s, double r, double sg, double& e, double& vr, double& vs) {
    const double cx = 0.9305257363491002;   // (3/2) (3 / (4 pi))^(1/3)
    const double c2 = 0.016455307846020558;  // 1 / (4 (6 pi^2)^(2/3))
    const double kappa = 0.804, mu = 0.2195149727645171;  // mu = beta pi^2 / 3, beta = 0.06672455060314922
    const double r13 = cbrt(r), r43 = r13 * r;
    const double p = c2 * sg / (r43 * r43);
    const double den = fma(mu, p, kappa);
    const double F = 1.0 + kappa * mu * p / den;
    const double dF = kappa * kappa * mu / (den * den);
    e += s * (-cx * r43 * F);
    vr += s * (-(4.0 / 3.0) * cx * r13 * (F - 2.0 * p * dF));
    vs += s * (-cx * c2 * dF / r43);
}

// Perdew and Wang's G(rs) = -2 A (1 + a1 rs) ln(1 + 1 / Q),  Q = 2 A (b1 x + b2 x^2 + b3 x^3 + b4 x^4),  x = sqrt(rs),
// and dG/drs = -2 A a1 ln(1 + 1 / Q) + 2 A (1 + a1 rs) Q' / (Q (Q + 1))
__device__ __forceinline__ void xc_pw_g(double x, double a, double a1, double b1, double b2, double b3, double b4, double& g,
                                        double& dg) {
    const double q = 2.0 * a * x * fma(x, fma(x, fma(x, b4, b3), b2), b1);
    const double dq = a * (b1 / x + fma(x, fma(4.0 * b4, x, 3.0 * b3), 2.0 * b2));
    const double l = log1p(1.0 / q);
    const double pre = -2.0 * a * fma(a1, x * x, 1.0);
    g = pre * l;
    dg = -2.0 * a * a1 * l - pre * dq / (q * (q + 1.0));
}

// The correlation energy per electron of Perdew and Wang 1992 with libxc's LDA_C_PW_MOD constants:
//   eps = eps0 + alpha_c f(zeta) / f''(0) (1 - zeta^4) + (eps1 - eps0) f(zeta) zeta^4
// with its derivatives with respect to rs and zeta, and what the gradient correction needs of the spin variables
struct XcPw {
    double rho, rs, up, dn, cp, cm;  // 1 +- zeta and their cube roots
    double eps, drs, dz;
};

__device__ __forceinline__ XcPw xc_pw_eps(double ra, double rb) {
    XcPw w;
    w.rho = ra + rb;
    const double zeta = (ra - rb) / w.rho;
    const double x = sqrt(cbrt(0.238732414637843 / w.rho));  // sqrt(rs), rs = (3 / (4 pi rho))^(1/3)
    w.rs = x * x;
    w.up = 2.0 * ra / w.rho, w.dn = 2.0 * rb / w.rho;  // 1 +- zeta, never by subtraction: zeta -> +-1 when a spin is empty
    w.cp = cbrt(w.up), w.cm = cbrt(w.dn);
    const double c43 = 0.5198420997897464;   // 2^(4/3) - 2
    const double fpp0 = 1.7099209341613657;  // 4 / (9 (2^(1/3) - 1)), exact
    const double fz = (w.cp * w.up + w.cm * w.dn - 2.0) / c43;
    const double dfz = (4.0 / 3.0) * (w.cp - w.cm) / c43;
    double e0, de0, e1, de1, ma, dma;  // ma = -alpha_c
    xc_pw_g(x, 0.0310907, 0.21370, 7.5957, 3.5876, 1.6382, 0.49294, e0, de0);
    xc_pw_g(x, 0.01554535, 0.20548, 14.1189, 6.1977, 3.3662, 0.62517, e1, de1);
    xc_pw_g(x, 0.0168869, 0.11125, 10.357, 3.6231, 0.88026, 0.49671, ma, dma);
    const double z3 = zeta * zeta * zeta, z4 = z3 * zeta;
    const double omz4 = w.up * w.dn * fma(zeta, zeta, 1.0);  // 1 - zeta^4 as a product of its factors
    w.eps = e0 - ma * fz / fpp0 * omz4 + (e1 - e0) * fz * z4;
    w.drs = de0 - dma * fz / fpp0 * omz4 + (de1 - de0) * fz * z4;
    w.dz = -ma / fpp0 * (dfz * omz4 - 4.0 * fz * z3) + (e1 - e0) * (dfz * z4 + 4.0 * fz * z3);
    return w;
}

// e = rho eps(rs, zeta):  d/d rho_s = eps - (rs / 3) d eps / d rs  +-  (1 -+ zeta) d eps / d zeta
__device__ __forceinline__ void xc_pw_mod(double s, double ra, double rb, XcDer& o) {
    const XcPw w = xc_pw_eps(ra, rb);
    const double common = w.eps - (w.rs / 3.0) * w.drs;
    o.e += s * w.rho * w.eps;
    o.va += s * (common + w.dn * w.dz);
    o.vb += s * (common - w.up * w.dz);
}

// Perdew-Burke-Ernzerhof correlation (libxc GGA_C_PBE): e = rho (eps + H),
//   H = gamma phi^3 ln(1 + X),  X = (beta / gamma) T (1 + y) / (1 + y + y^2),  y = A T,  A = (beta / gamma) / em,
//   em = exp(u) - 1,  u = -eps / (gamma phi^3),  phi = ((1 + zeta)^(2/3) + (1 - zeta)^(2/3)) / 2,
//   T = t^2 = sigma / (4 phi^2 k_s^2 rho^2) = pi sigma / (16 (3 pi^2)^(1/3) phi^2 rho^(7/3))
// X = em (y + y^2) / (1 + y + y^2) = em (1 - 1 / (1 + y + y^2)): the second form where y > 1 (y reaches 1e7 at a large
// reduced gradient, where H -> -eps).  With D = 1 + y + y^2:
//   dX/dT (A fixed) = (beta / gamma) (1 + 2 y) / D^2,   dX/du (T fixed) = y^3 (2 + y) (1 + em) / D^2,
//   dH = 3 gamma phi^2 ln(1 + X) dphi + gamma phi^3 / (1 + X) dX,
//   du = -d eps / (gamma phi^3) - 3 u dphi / phi,   dT = T (d sigma / sigma - 2 dphi / phi - (7/3) d rho / rho)
// expm1 and log1p: eps -> 0 in the density tails.  dphi/dzeta = ((1 + zeta)^(-1/3) - (1 - zeta)^(-1/3)) / 3 is finite
// because the densities are clamped at rho_floor / 2.
__device__ __forceinline__ void xc_pbe_c(double s, double ra, double rb, double saa, double sab, double sbb, XcDer& o) {
    const double gamma = 0.031090690869654895;  // (1 - ln 2) / pi^2
    const double bg = 2.1461263399673646;       // beta / gamma, beta = 0.06672455060314922
    const double ct = 0.0634682060977037;       // pi / (16 (3 pi^2)^(1/3))
    const XcPw w = xc_pw_eps(ra, rb);
    const double phi = 0.5 * (w.cp * w.cp + w.cm * w.cm);
    const double dphi = (1.0 / w.cp - 1.0 / w.cm) / 3.0;
    const double phi2 = phi * phi, g3 = gamma * phi2 * phi;
    const double kt = ct / (phi2 * w.rho * w.rho * cbrt(w.rho));  // T = kt sigma
    const double T = kt * (saa + 2.0 * sab + sbb);
    const double em = expm1(-w.eps / g3);
    const double y = bg / em * T;
    const double D = fma(y, y + 1.0, 1.0), D2 = D * D;
    const double X = em * (y > 1.0 ? 1.0 - 1.0 / D : y * (1.0 + y) / D);
    const double L = log1p(X);
    const double H = g3 * L;
    const double hx = g3 / (1.0 + X);                              // dH/dX
    const double XT = bg * fma(2.0, y, 1.0) / D2;                  // dX/dT
    const double q = y * y * y * (2.0 + y) * (1.0 + em) / D2 / (1.0 + X);  // (dH/dX) (dX/du) / (gamma phi^3)
    const double vs = w.rho * hx * XT * kt;                        // d(rho H) / d sigma
    // d(rho H)/d rho at fixed zeta (d eps / d rho = -(rs / (3 rho)) d eps / d rs), and dH/dzeta (gamma phi^3 u = -eps)
    const double Hn = H - (7.0 / 3.0) * hx * XT * T + q * w.rs * w.drs / 3.0;
    const double Hz = (3.0 * gamma * phi2 * L - 2.0 * hx * XT * T / phi + 3.0 * q * w.eps / phi) * dphi - q * w.dz;
    const double common = w.eps - (w.rs / 3.0) * w.drs + Hn;
    const double dz = w.dz + Hz;
    o.e += s * w.rho * (w.eps + H);
    o.va += s * (common + w.dn * dz);
    o.vb += s * (common - w.up * dz);
    o.vaa += s * vs;
    o.vab += s * 2.0 * vs;
    o.vbb += s * vs;
}

// Conventions (nbed_amd.xc, "Meta-GGA conventions"): wherever z = tau_W / tau is formed, tau is clamped from below at
// tau_W = sigma / (8 n) of the same clamped quantities by the test tau >= sigma / (8 n) * XC_TPSS_CLAMP; where it fails
// z = 1 and alpha = 0 are constants.  XC_TPSS_CLAMP = 1 - 1e-10: a one-orbital density has tau = tau_W at every point up
// to the rounding of the density pass, and the potential has a kink at the clamp -- the margin keeps such points on one
// side of it (z <= 1 + 1e-10).  "The larger of" a and b is a where a >= b.
//
// TPSS exchange of one spin channel (spin-scaled: E_x[n_a, n_b] = 1/2 E_x[2 n_a] + 1/2 E_x[2 n_b], tau doubled too):
//   e = -cx rho^(4/3) F(p, z),  F = 1 + kappa - kappa / (1 + x / kappa) = 1 + kappa x / (kappa + x),
//   p = sigma / (4 (6 pi^2)^(2/3) rho^(8/3)),  z = sigma / (8 rho tau),
//   alpha = (5p/3)(1/z - 1) = (tau - tau_W) / (cF rho^(5/3)),  cF = (3/10)(6 pi^2)^(2/3)   (no 0 x inf at a zero gradient)
//   q_b = (9/20)(alpha - 1) / sqrt(1 + b alpha (alpha - 1)) + 2p/3
//   x = N / (1 + sqrt(e) p)^2,  N = [10/81 + c z^2 / (1 + z^2)^2] p + (146/2025) q_b^2 - (73/405) q_b sqrt((9/50) z^2 + p^2/2)
//       + (10/81)^2 p^2 / kappa + 2 sqrt(e) (10/81) (9/25) z^2 + e mu p^3
// The chain rule runs through (p, z, alpha), each with its derivatives with respect to (rho, sigma, tau).
constexpr double XC_TPSS_CLAMP = 1.0 - 1e-10;

__device__ __forceinline__ void xc_tpss_x(double s, double r, double sg, double tau, double& e, double& vr, double& vs,
                                          double& vt) {
    const double cx = 0.9305257363491002;    // (3/2) (3 / (4 pi))^(1/3)
    const double c2 = 0.016455307846020558;  // 1 / (4 (6 pi^2)^(2/3))
    const double cf = 4.557799872345596;     // (3/10) (6 pi^2)^(2/3)
    const double kappa = 0.804, b = 0.40, c = 1.59096, ee = 1.537, mu = 0.21951;
    const double se = 1.239758040909596;     // sqrt(e)
    const double k1 = 146.0 / 2025.0, k2 = 73.0 / 405.0, k3 = (10.0 / 81.0) * (10.0 / 81.0) / kappa;
    const double k4 = 2.0 * se * (10.0 / 81.0) * 0.36, k5 = ee * mu;
    const double r13 = cbrt(r), r43 = r13 * r, r53 = r13 * r13 * r, r83 = r43 * r43;
    const double p = c2 * sg / r83;
    const double tw = sg / (8.0 * r);
    double z = 1.0, alpha = 0.0, z_r = 0.0, z_s = 0.0, z_t = 0.0, a_r = 0.0, a_s = 0.0, a_t = 0.0;
    if (tau >= tw * XC_TPSS_CLAMP) {
        z = tw / tau;
        a_t = 1.0 / (cf * r53);
        alpha = (tau - tw) * a_t;
        z_r = -z / r, z_s = 1.0 / (8.0 * r * tau), z_t = -z / tau;
        a_s = -a_t / (8.0 * r);
        a_r = (tw / r) * a_t - (5.0 / 3.0) * alpha / r;
    }
    const double z2 = z * z, am1 = alpha - 1.0;
    const double w = fma(b * alpha, am1, 1.0), sw = sqrt(w);
    const double qb = 0.45 * am1 / sw + (2.0 / 3.0) * p;
    // d/dalpha of (alpha - 1) / sqrt(w) is (1 - b / 2 + b alpha / 2) / w^(3/2): as 1 / sqrt(w) - (alpha - 1) w' / (2 w^(3/2))
    // its two terms cancel to 1 / alpha of their size
    const double qb_a = 0.45 * fma(0.5 * b, alpha, 1.0 - 0.5 * b) / (w * sw);
    const double opz = 1.0 + z2;
    const double t1 = 10.0 / 81.0 + c * z2 / (opz * opz);
    const double t1_z = 2.0 * c * z * (1.0 - z2) / (opz * opz * opz);
    const double sq = sqrt(fma(0.18, z2, 0.5 * p * p));
    const double sq_z = 0.18 * z / sq, sq_p = 0.5 * p / sq;
    const double lin = 2.0 * k1 * qb - k2 * sq;  // dN/dq_b
    const double N = t1 * p + k1 * qb * qb - k2 * qb * sq + k3 * p * p + k4 * z2 + k5 * p * p * p;
    const double N_p = t1 + (2.0 / 3.0) * lin - k2 * qb * sq_p + 2.0 * k3 * p + 3.0 * k5 * p * p;
    const double N_z = t1_z * p - k2 * qb * sq_z + 2.0 * k4 * z;
    const double N_a = lin * qb_a;
    const double d1 = fma(se, p, 1.0), Dn = d1 * d1;
    const double x = N / Dn;
    const double x_p = N_p / Dn - 2.0 * se * x / d1, x_z = N_z / Dn, x_a = N_a / Dn;
    const double kx = kappa + x;
    const double F = 1.0 + kappa * x / kx, Fx = kappa * kappa / (kx * kx);
    const double dF_r = Fx * (x_p * (-(8.0 / 3.0) * p / r) + x_z * z_r + x_a * a_r);
    const double dF_s = Fx * (x_p * (c2 / r83) + x_z * z_s + x_a * a_s);
    const double dF_t = Fx * (x_z * z_t + x_a * a_t);
    e += s * (-cx * r43 * F);
    vr += s * (-cx * ((4.0 / 3.0) * r13 * F + r43 * dF_r));
    vs += s * (-cx * r43 * dF_s);
    vt += s * (-cx * r43 * dF_t);
}

// eps_PBE(n_s, 0, grad n_s, 0) per electron with its derivatives with respect to (n_s, sigma_ss): xc_pbe_c at zeta = 1
// written without the empty channel (f(zeta) = 1, zeta^4 = 1, 1 - zeta^4 = 0: eps_PW = eps_1; phi = 2^(-1/3)), so that
// nothing is differentiated with respect to it.
__device__ __forceinline__ void xc_pbe_c_pol(double r, double sg, double& eps, double& d_r, double& d_s) {
    const double gamma = 0.031090690869654895, bg = 2.1461263399673646, ct = 0.0634682060977037;
    const double phi2 = 0.6299605249474366;  // 2^(-2/3)
    const double g3 = 0.5 * gamma;
    const double x = sqrt(cbrt(0.238732414637843 / r));
    const double rs = x * x;
    double e1, de1;
    xc_pw_g(x, 0.01554535, 0.20548, 14.1189, 6.1977, 3.3662, 0.62517, e1, de1);
    const double kt = ct / (phi2 * r * r * cbrt(r));
    const double T = kt * sg;
    const double em = expm1(-e1 / g3);
    const double y = bg / em * T;
    const double D = fma(y, y + 1.0, 1.0), D2 = D * D;
    const double X = em * (y > 1.0 ? 1.0 - 1.0 / D : y * (1.0 + y) / D);
    const double H = g3 * log1p(X);
    const double hx = g3 / (1.0 + X);
    const double XT = bg * fma(2.0, y, 1.0) / D2;
    const double q = y * y * y * (2.0 + y) * (1.0 + em) / D2 / (1.0 + X);
    eps = e1 + H;
    d_s = hx * XT * kt;
    d_r = (-(rs / 3.0) * de1 - (7.0 / 3.0) * hx * XT * T + q * rs * de1 / 3.0) / r;
}

// TPSS correlation: e = n eps (1 + d eps z^3) with eps = eps_revPKZB,
//   eps_revPKZB = eps_PBE (1 + C z^2) - (1 + C) z^2 sum_s (n_s / n) max(eps_PBE(n_s, 0, grad n_s, 0), eps_PBE),
//   z = sigma / (8 n tau) of the totals,  C = (0.53 + 0.87 zeta^2 + 0.50 zeta^4 + 2.26 zeta^6) / (1 + X)^4,
//   X = xi^2 ((1 + zeta)^(-4/3) + (1 - zeta)^(-4/3)) / 2 = Q h / (2 (3 pi^2)^(2/3) n^(14/3)),
//   Q = n_b^2 sigma_aa - 2 n_a n_b sigma_ab + n_a^2 sigma_bb (= n^4 |grad zeta|^2 / 4),  h = up^(-4/3) + dn^(-4/3),
// 1 +- zeta = 2 n_s / n never by subtraction; C is the fourth power of 1 / (1 + X): where a fully polarised point has a
// gradient of zeta, X is 1e18 and C underflows towards 0 with finite derivatives.  d[0..5]: the derivatives of e with
// respect to (n_a, n_b, sigma_aa, sigma_ab, sigma_bb, tau); eps_PBE and its derivatives come from xc_pbe_c.
__device__ __forceinline__ void xc_tpss_c(double ra, double rb, double saa, double sab, double sbb, double tau, double& e,
                                          double (&d)[6]) {
    const double dd = 2.8;
    XcDer P = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    xc_pbe_c(1.0, ra, rb, saa, sab, sbb, P);
    const double n = ra + rb, n2 = n * n;
    const double E = P.e / n;
    const double dE[6] = {(P.va - E) / n, (P.vb - E) / n, P.vaa / n, P.vab / n, P.vbb / n, 0.0};
    double Ea, Ea_r, Ea_s, Eb, Eb_r, Eb_s;
    xc_pbe_c_pol(ra, saa, Ea, Ea_r, Ea_s);
    xc_pbe_c_pol(rb, sbb, Eb, Eb_r, Eb_s);
    const bool sa = Ea >= E, sb = Eb >= E;
    const double A = sa ? Ea : E, B = sb ? Eb : E;
    const double fa = ra / n, fb = rb / n;
    const double S = fa * A + fb * B;
    // z of the totals
    const double st = saa + 2.0 * sab + sbb;
    const double tw = st / (8.0 * n);
    double z = 1.0, dz[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (tau >= tw * XC_TPSS_CLAMP) {
        const double zk = 1.0 / (8.0 * n * tau);
        z = st * zk;
        dz[0] = dz[1] = -z / n;
        dz[2] = dz[4] = zk;
        dz[3] = 2.0 * zk;
        dz[5] = -z / tau;
    }
    const double z2 = z * z, z3 = z2 * z;
    // C(zeta, xi)
    const double zeta = (ra - rb) / n, up = 2.0 * ra / n, dn = 2.0 * rb / n, zz = zeta * zeta;
    const double num = fma(zz, fma(zz, fma(zz, 2.26, 0.50), 0.87), 0.53);
    const double dnum = zeta * fma(zz, fma(zz, 13.56, 2.0), 1.74);
    const double dzeta[2] = {dn / n, -up / n};
    const double Q = rb * rb * saa - 2.0 * ra * rb * sab + ra * ra * sbb;
    const double hu = 1.0 / (cbrt(up) * up), hd = 1.0 / (cbrt(dn) * dn);
    const double h = hu + hd;
    const double h_up = -(4.0 / 3.0) * hu / up, h_dn = -(4.0 / 3.0) * hd / dn;
    const double dh[2] = {(h_up - h_dn) * dn / n, (h_dn - h_up) * up / n};
    const double cn = cbrt(n);
    const double gq = 1.0 / (19.141560001254607 * n2 * n2 * cn * cn);  // 1 / (2 (3 pi^2)^(2/3) n^(14/3))
    const double X = Q * h * gq;
    const double dQ[2] = {2.0 * (ra * sbb - rb * sab), 2.0 * (rb * saa - ra * sab)};
    const double dX[6] = {(dQ[0] * h + Q * dh[0]) * gq - (14.0 / 3.0) * X / n, (dQ[1] * h + Q * dh[1]) * gq - (14.0 / 3.0) * X / n,
                          rb * rb * h * gq, -2.0 * ra * rb * h * gq, ra * ra * h * gq, 0.0};
    const double inv = 1.0 / (1.0 + X), inv2 = inv * inv, i4 = inv2 * inv2;
    const double C = num * i4;
    const double rev = E * fma(C, z2, 1.0) - (1.0 + C) * z2 * S;
    const double g1 = fma(2.0 * dd * rev, z3, 1.0);
    const double eps = rev * fma(dd * rev, z3, 1.0);
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const double dC = (i < 2 ? dnum * dzeta[i] * i4 : 0.0) - 4.0 * C * inv * dX[i];
        double dA = sa ? 0.0 : dE[i], dB = sb ? 0.0 : dE[i];
        if (sa && i == 0) dA = Ea_r;
        if (sa && i == 2) dA = Ea_s;
        if (sb && i == 1) dB = Eb_r;
        if (sb && i == 4) dB = Eb_s;
        double dS = fa * dA + fb * dB;
        if (i == 0) dS += rb / n2 * (A - B);
        if (i == 1) dS += ra / n2 * (B - A);
        const double dz2 = 2.0 * z * dz[i];
        const double drev = dE[i] * fma(C, z2, 1.0) + E * (dC * z2 + C * dz2) - (dC * z2 + (1.0 + C) * dz2) * S -
                            (1.0 + C) * z2 * dS;
        const double deps = drev * g1 + dd * rev * rev * 3.0 * z2 * dz[i];
        d[i] = n * deps + (i < 2 ? eps : 0.0);
    }
    e = n * eps;
}

constexpr int XC_FN_THREADS = 256;

// CODE: NBX_XC_SLATER / _LDA_VWN_RPA / _LDA_VWN5 / _B3LYP / _LDA_PW_MOD / _PBE / _PBEH / _BLYP / _B3LYP5, the
// range-separated NBX_XC_CAM_B3LYP / _LC_BLYP of nbx_xc_functional_rs, which alone read `omega` (the semi-local
// part; the exact-exchange fractions are the caller's), and the meta-GGAs NBX_XC_TPSS / _TPSSH (0.9 of the exchange;
// the 0.1 of exact exchange is the caller's) of nbx_xc_functional_mgga, which alone read `tau` (2, npts) and write `vt`
// (both null otherwise, and last, so that the other codes find their arguments where they were without them);
// one instantiation each: a kernel holding every branch would charge the registers of the heaviest code to all of them
// (the meta-GGAs take all 256 VGPRs, the LDA codes 52).  Conventions of nbed_amd.xc.XCProvider.__call__ (the torch
// expression this kernel replaces): densities clamped from below at rho_floor / 2, sigma_aa and sigma_bb lifted by
// 1e-40, points with rho_a + rho_b <= rho_floor dropped; the TPSS exchange clamps each channel's tau against its own
// tau_W, the correlation tau_a + tau_b against the total's; outputs carry the quadrature weights:
//   vr[x][g]     = w keep dE/drho_x
//   vec[x][a][g] = w keep (2 dE/dsigma_xx grad rho_x + dE/dsigma_ab grad rho_other)[a]
//   vt[x][g]     = w keep dE/dtau_x                                                        (meta-GGAs)
//   part[blk]    = (sum w keep e, sum w (rho_a + rho_b)) of the block
template <int CODE>
__global__ __launch_bounds__(XC_FN_THREADS) void xc_functional_kernel(int64_t npts, const double* __restrict__ rho,
                                                                      const double* __restrict__ grad,
                                                                      const double* __restrict__ w, double rho_floor,
                                                                      double omega, double* __restrict__ vr,
                                                                      double* __restrict__ vec, double* __restrict__ part,
                                                                      const double* __restrict__ tau,
                                                                      double* __restrict__ vt) {
    constexpr bool MGGA = CODE == NBX_XC_TPSS || CODE == NBX_XC_TPSSH;
    __shared__ double red[17];
    const int64_t g = (int64_t)blockIdx.x * XC_FN_THREADS + threadIdx.x;
    double e_w = 0.0, n_w = 0.0;
    if (g < npts) {
        const double r0 = rho[g], r1 = rho[npts + g], wg = w[g];
        const double gax = grad[g], gay = grad[npts + g], gaz = grad[2 * npts + g];
        const double gbx = grad[3 * npts + g], gby = grad[4 * npts + g], gbz = grad[5 * npts + g];
        n_w = wg * (r0 + r1);
        const double keep = (r0 + r1) > rho_floor ? 1.0 : 0.0;
        const double ra = fmax(r0, 0.5 * rho_floor), rb = fmax(r1, 0.5 * rho_floor);
        const double saa = fma(gax, gax, fma(gay, gay, gaz * gaz)) + 1.0e-40;
        const double sbb = fma(gbx, gbx, fma(gby, gby, gbz * gbz)) + 1.0e-40;
        const double sab = fma(gax, gbx, fma(gay, gby, gaz * gbz));
        XcDer o = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        double vta = 0.0, vtb = 0.0;  // dE/dtau_x (meta-GGAs)
        if constexpr (MGGA) {
            const double ax = CODE == NBX_XC_TPSS ? 1.0 : 0.9, ta = tau[g], tb = tau[npts + g];
            xc_tpss_x(ax, ra, saa, ta, o.e, o.va, o.vaa, vta);
            xc_tpss_x(ax, rb, sbb, tb, o.e, o.vb, o.vbb, vtb);
            double ec, dc[6];
            xc_tpss_c(ra, rb, saa, sab, sbb, ta + tb, ec, dc);
            o.e += ec, o.va += dc[0], o.vb += dc[1], o.vaa += dc[2], o.vab += dc[3], o.vbb += dc[4];
            vta += dc[5], vtb += dc[5];
        } else if (CODE == NBX_XC_SLATER) {
            xc_slater(1.0, ra, rb, o);
        } else if (CODE == NBX_XC_LDA_VWN_RPA) {
            xc_slater(1.0, ra, rb, o);
            xc_vwn<true>(1.0, ra, rb, o);
        } else if (CODE == NBX_XC_LDA_VWN5) {
            xc_slater(1.0, ra, rb, o);
            xc_vwn<false>(1.0, ra, rb, o);
        } else if (CODE == NBX_XC_B3LYP || CODE == NBX_XC_B3LYP5) {
            xc_slater(0.8, ra, rb, o);
            xc_b88(0.72, ra, saa, o.e, o.va, o.vaa);
            xc_b88(0.72, rb, sbb, o.e, o.vb, o.vbb);
            xc_vwn<CODE == NBX_XC_B3LYP>(0.19, ra, rb, o);
            xc_lyp(0.81, ra, rb, saa, sab, sbb, o);
        } else if (CODE == NBX_XC_LDA_PW_MOD) {
            xc_slater(1.0, ra, rb, o);
            xc_pw_mod(1.0, ra, rb, o);
        } else if (CODE == NBX_XC_PBE || CODE == NBX_XC_PBEH) {
            const double ax = CODE == NBX_XC_PBE ? 1.0 : 0.75;
            xc_pbe_x(ax, ra, saa, o.e, o.va, o.vaa);
            xc_pbe_x(ax, rb, sbb, o.e, o.vb, o.vbb);
            xc_pbe_c(1.0, ra, rb, saa, sab, sbb, o);
        } else if (CODE == NBX_XC_CAM_B3LYP) {  // (1 - 0.19 - 0.46) B88 + 0.46 B88^sr(omega) + 0.81 LYP + 0.19 VWN5
            xc_slater(0.35, ra, rb, o);
            xc_b88(0.35, ra, saa, o.e, o.va, o.vaa);
            xc_b88(0.35, rb, sbb, o.e, o.vb, o.vbb);
            xc_b88_sr(0.46, omega, ra, saa, o.e, o.va, o.vaa);
            xc_b88_sr(0.46, omega, rb, sbb, o.e, o.vb, o.vbb);
            xc_vwn<false>(0.19, ra, rb, o);
            xc_lyp(0.81, ra, rb, saa, sab, sbb, o);
        } else if (CODE == NBX_XC_LC_BLYP) {  // B88^sr(omega) + LYP
            xc_b88_sr(1.0, omega, ra, saa, o.e, o.va, o.vaa);
            xc_b88_sr(1.0, omega, rb, sbb, o.e, o.vb, o.vbb);
            xc_lyp(1.0, ra, rb, saa, sab, sbb, o);
        } else {  // BLYP
            xc_slater(1.0, ra, rb, o);
            xc_b88(1.0, ra, saa, o.e, o.va, o.vaa);
            xc_b88(1.0, rb, sbb, o.e, o.vb, o.vbb);
            xc_lyp(1.0, ra, rb, saa, sab, sbb, o);
        }
        const double wk = wg * keep;
        e_w = wk * o.e;
        vr[g] = wk * o.va;
        vr[npts + g] = wk * o.vb;
        if constexpr (MGGA) {
            vt[g] = wk * vta;
            vt[npts + g] = wk * vtb;
        }
        const double a2 = 2.0 * wk * o.vaa, b2 = 2.0 * wk * o.vbb, ab = wk * o.vab;
        vec[g] = fma(a2, gax, ab * gbx);
        vec[npts + g] = fma(a2, gay, ab * gby);
        vec[2 * npts + g] = fma(a2, gaz, ab * gbz);
        vec[3 * npts + g] = fma(b2, gbx, ab * gax);
        vec[4 * npts + g] = fma(b2, gby, ab * gay);
        vec[5 * npts + g] = fma(b2, gbz, ab * gaz);
    }
    const double es = nbx_block_sum(e_w, red);
    const double ns = nbx_block_sum(n_w, red);
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = es;
        part[2 * blockIdx.x + 1] = ns;
    }
}

// sums the block partials in a fixed order (one workgroup): out[0] = E_xc, out[1] = integrated electron count
__global__ __launch_bounds__(256) void xc_sums_kernel(int nblk, const double* __restrict__ part, double* __restrict__ out) {
    __shared__ double red[17];
    double e = 0.0, n = 0.0;
    for (int i = threadIdx.x; i < nblk; i += 256) {
        e += part[2 * i];
        n += part[2 * i + 1];
    }
    e = nbx_block_sum(e, red);
    n = nbx_block_sum(n, red);
    if (threadIdx.x == 0) {
        out[0] = e;
        out[1] = n;
    }
}

// ------------------------------------------------------------------------------------------------ potential pass
// Workgroup = BT waves; block (bm, bn) of the (nao x nao) result, 16 BT rows and columns; wave w owns tile row w of
// the block and all BT column tiles.  Grid points are consumed 16 at a time: the threads build the 16 x (16 BT)
// tile of `half` into LDS (double buffered: one barrier per step), every wave multiplies its ao^T fragments (read
// straight from global memory: 16 consecutive AO columns per grid point) with it.
// TAU (`vt` is read by no other instantiation; null there): four products per step of 16 grid points, all into the same
// accumulators: operand 0 is the plain step, A = ao against B = half; operands 1 .. 3 are A = dao_a against
// B = 1/4 vt dao_a for a = x, y, z, each B built on the fly.  The (step, operand) pairs run through the same
// double-buffered LDS tile as one sequence four times as long: no more LDS, one barrier per product.  With vt = 0 the
// three extra products add zeros: the plain kernel's bits.
template <int BT, bool TAU>
__global__ __launch_bounds__(64 * BT) void xc_vmat_kernel(int64_t npts, int nao, int64_t chunk, int nblk,
                                                          const double* __restrict__ ao, const double* __restrict__ dao,
                                                          const double* __restrict__ vr, const double* __restrict__ vec,
                                                          double* __restrict__ part, const double* __restrict__ vt) {
    constexpr int W = 16 * BT, LD = (W % 32 == 16) ? W : W + 16, NT = 64 * BT;
    __shared__ __attribute__((aligned(16))) double hs[2][16 * LD];
    const int x = blockIdx.z;
    const int bm = blockIdx.y / nblk, bn = blockIdx.y - bm * nblk;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fr = lane & 15, fk = lane >> 4;
    const int64_t g_begin = (int64_t)blockIdx.x * chunk, g_end = min(npts, g_begin + chunk);
    const int64_t plane = npts * (int64_t)nao;
    const double* vrx = vr + (int64_t)x * npts;
    const double* vcx = vec + (int64_t)(3 * x) * npts;
    const double* vtx = TAU ? vt + (int64_t)x * npts : nullptr;
    const int m = W * bm + 16 * wave + fr;  // the A-fragment column of ao / dao_a (row of the result) of this lane
    const bool m_ok = m < nao;
    xc_v4 acc[BT];
#pragma unroll
    for (int c = 0; c < BT; ++c) acc[c] = (xc_v4){0.0, 0.0, 0.0, 0.0};

    auto produce = [&](int buf, int64_t g0, int op) {  // the B tile of operand `op` at the 16 points from g0 on
#pragma unroll
        for (int i = 0; i < 4; ++i) {  // 16 W elements over NT = 4 W threads
            const int e = threadIdx.x + i * NT;
            const int gl = e / W, nl = e - gl * W;
            const int64_t g = g0 + gl;
            const int n = W * bn + nl;
            double h = 0.0;
            if (g < g_end && n < nao) {
                const int64_t off = g * nao + n;
                if (!TAU || op == 0)
                    h = fma(0.5 * vrx[g], ao[off],
                            fma(vcx[g], dao[off], fma(vcx[npts + g], dao[plane + off], vcx[2 * npts + g] * dao[2 * plane + off])));
                else
                    h = 0.25 * vtx[g] * dao[(op - 1) * plane + off];
            }
            hs[buf][gl * LD + nl] = h;
        }
    };

    // One product per pass of the loop.  Plain: one per step, and s is the step's first grid point.  TAU: four per step,
    // and s counts the (step, operand) pairs.  (Written so that the plain loop runs over g0 itself: counted in steps it
    // compiles to other, longer code.)
    constexpr int DS = TAU ? 1 : 16;
    const int64_t s_begin = TAU ? 0 : g_begin;
    const int64_t s_end = TAU ? (g_begin < g_end ? 4 * ((g_end - g_begin + 15) / 16) : 0) : g_end;
    int buf = 0;
    if (s_begin < s_end) produce(0, g_begin, 0);
    for (int64_t s = s_begin; s < s_end; s += DS) {
        const int64_t g0 = TAU ? g_begin + 16 * (s >> 2) : s;
        const int op = TAU ? (int)(s & 3) : 0;
        __syncthreads();  // hs[buf] is complete; hs[buf ^ 1] has been consumed
        if (s + DS < s_end) produce(buf ^ 1, TAU ? g_begin + 16 * ((s + 1) >> 2) : s + 16, TAU ? (int)((s + 1) & 3) : 0);
        const double* src = op == 0 ? ao : dao + (op - 1) * plane;
        double a[4];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const int64_t g = g0 + 4 * kk + fk;
            a[kk] = (m_ok && g < g_end) ? src[g * nao + m] : 0.0;
        }
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
            for (int c = 0; c < BT; ++c)
                acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[kk], hs[buf][(4 * kk + fk) * LD + 16 * c + fr], acc[c], 0, 0, 0);
        buf ^= 1;
    }
    // this chunk's contribution to the block: part[chunk][x][row][col]
    double* out = part + ((int64_t)blockIdx.x * 2 + x) * (int64_t)nao * nao;
#pragma unroll
    for (int c = 0; c < BT; ++c) {
        const int col = W * bn + 16 * c + fr;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = W * bm + 16 * wave + fk + 4 * r;
            if (row < nao && col < nao) out[(int64_t)row * nao + col] = acc[c][r];
        }
    }
}

// v[x][m][n] = sum_chunks (part[c][x][m][n] + part[c][x][n][m]), chunks in ascending order
__global__ __launch_bounds__(256) void xc_vmat_reduce_kernel(int nao, int nchunk, const double* __restrict__ part,
                                                             double* __restrict__ v) {
    const int64_t n2 = (int64_t)nao * nao;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * n2) return;
    const int x = (int)(i / n2);
    const int64_t e = i - x * n2;
    const int m = (int)(e / nao), n = (int)(e - (int64_t)m * nao);
    const int64_t et = (int64_t)n * nao + m;
    double s = 0.0;
    for (int c = 0; c < nchunk; ++c) {
        const double* p = part + ((int64_t)c * 2 + x) * n2;
        s += p[e] + p[et];
    }
    v[i] = s;
}

int vmat_bt(int64_t nao) {  // tiles per block side: the least padded 16 BT grid over nao, the larger BT on a tie
    int best = 1;
    int64_t best_pad = -1;
    for (int bt = 1; bt <= 5; ++bt) {
        const int64_t w = 16 * bt, pad = nbx_cdiv(nao, w) * w;
        if (best_pad < 0 || pad <= best_pad) {
            best = bt;
            best_pad = pad;
        }
    }
    return best;
}

int64_t vmat_chunk(int64_t npts, int64_t nao) {  // grid points per workgroup: enough workgroups to fill the chip
    const int bt = vmat_bt(nao);
    const int64_t nblk = nbx_cdiv(nao, 16 * bt);
    int64_t chunk = 2048;
    while (chunk > 256 && nbx_cdiv(npts, chunk) * nblk * nblk * 2 < 1024) chunk >>= 1;
    return chunk;
}

size_t xc_align256(size_t x) { return (x + 255) & ~(size_t)255; }

// nbx_xc_rho (d_tau = nullptr) and nbx_xc_rho_tau (`who` names the one for the error text); the other arguments are
// checked here
int xc_rho_launch(const char* who, nbx_ctx* ctx, int64_t npts, int64_t nao, const double* d_ao, const double* d_dao,
                  const double* d_dm, double* d_rho, double* d_grad, double* d_tau) {
    NBX_CHECK_ARG(ctx && d_ao && d_dao && d_dm && d_rho && d_grad && npts >= 0 && nao >= 1);
    const int64_t kp = (nao + 3) & ~3ll;
    const size_t lds = (size_t)(2 * kp * 16) * sizeof(double);
    if (lds > 160 * 1024) {
        nbx_set_error("%s: nao = %lld beyond the LDS-resident density slab (limit 640)", who, (long long)nao);
        return NBX_E_UNSUPPORTED;
    }
    if (npts == 0) return NBX_OK;
    // [the ao fragments stay in registers: nao <= 160][tau]
    static const decltype(&xc_rho_kernel<0, false>) kernels[2][2] = {{xc_rho_kernel<0, false>, xc_rho_kernel<0, true>},
                                                                     {xc_rho_kernel<40, false>, xc_rho_kernel<40, true>}};
    static bool attr_set = false;
    if (!attr_set) {
        for (int i = 0; i < 4; ++i)
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernels[i >> 1][i & 1]),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        attr_set = true;
    }
    hipLaunchKernelGGL(kernels[kp <= 160][d_tau != nullptr], dim3((unsigned)nbx_cdiv(npts, 64)), dim3(256), lds, ctx->stream,
                       npts, (int)nao, d_ao, d_dao, d_dm, d_rho, d_grad, d_tau);
    NBX_LAUNCH_CHECK();
    return NBX_OK;
}

}  // namespace

extern "C" int nbx_xc_rho(nbx_ctx* ctx, int64_t npts, int64_t nao, const double* d_ao, const double* d_dao,
                          const double* d_dm, double* d_rho, double* d_grad) {
    return xc_rho_launch("nbx_xc_rho", ctx, npts, nao, d_ao, d_dao, d_dm, d_rho, d_grad, nullptr);
}

extern "C" int nbx_xc_rho_tau(nbx_ctx* ctx, int64_t npts, int64_t nao, const double* d_ao, const double* d_dao,
                              const double* d_dm, double* d_rho, double* d_grad, double* d_tau) {
    NBX_CHECK_ARG(d_tau);
    return xc_rho_launch("nbx_xc_rho_tau", ctx, npts, nao, d_ao, d_dao, d_dm, d_rho, d_grad, d_tau);
}

extern "C" size_t nbx_xc_functional_worksize(int64_t npts) {
    return npts <= 0 ? 256 : xc_align256((size_t)(2 * nbx_cdiv(npts, XC_FN_THREADS)) * sizeof(double));
}

namespace {

// nbx_xc_functional (codes 0 .. 8), nbx_xc_functional_rs (16, 17: the only ones that read omega) and
// nbx_xc_functional_mgga (32, 33: the only ones that read d_tau and write d_vt); the other arguments are checked here
int xc_functional_launch(nbx_ctx* ctx, int code, double omega, int64_t npts, const double* d_rho, const double* d_grad,
                         const double* d_tau, const double* d_w, double rho_floor, double* d_vr, double* d_vec, double* d_vt,
                         double* d_sums, void* d_work, size_t work_bytes) {
    NBX_CHECK_ARG(ctx && d_rho && d_grad && d_w && d_vr && d_vec && d_sums && d_work && npts >= 0);
    NBX_CHECK_ARG(rho_floor > 0.0 && work_bytes >= nbx_xc_functional_worksize(npts));
    if (npts == 0) return nbx_memset(ctx, d_sums, 0, 2 * sizeof(double));
    const int64_t nblk = nbx_cdiv(npts, XC_FN_THREADS);
    NBX_CHECK_ARG(nblk < (1ll << 30));
    double* part = static_cast<double*>(d_work);
#define NBX_XC_FN(CODE_)                                                                                                  \
    case CODE_:                                                                                                           \
        hipLaunchKernelGGL(xc_functional_kernel<CODE_>, dim3((unsigned)nblk), dim3(XC_FN_THREADS), 0, ctx->stream, npts,  \
                           d_rho, d_grad, d_w, rho_floor, omega, d_vr, d_vec, part, d_tau, d_vt);                         \
        break
    switch (code) {
        NBX_XC_FN(NBX_XC_SLATER);
        NBX_XC_FN(NBX_XC_LDA_VWN_RPA);
        NBX_XC_FN(NBX_XC_LDA_VWN5);
        NBX_XC_FN(NBX_XC_B3LYP);
        NBX_XC_FN(NBX_XC_LDA_PW_MOD);
        NBX_XC_FN(NBX_XC_PBE);
        NBX_XC_FN(NBX_XC_PBEH);
        NBX_XC_FN(NBX_XC_BLYP);
        NBX_XC_FN(NBX_XC_B3LYP5);
        NBX_XC_FN(NBX_XC_CAM_B3LYP);
        NBX_XC_FN(NBX_XC_LC_BLYP);
        NBX_XC_FN(NBX_XC_TPSS);
        default: NBX_XC_FN(NBX_XC_TPSSH);
    }
#undef NBX_XC_FN
    NBX_LAUNCH_CHECK();
    hipLaunchKernelGGL(xc_sums_kernel, dim3(1), dim3(256), 0, ctx->stream, (int)nblk, part, d_sums);
    NBX_LAUNCH_CHECK();
    return NBX_OK;
}

}  // namespace

extern "C" int nbx_xc_functional(nbx_ctx* ctx, int code, int64_t npts, const double* d_rho, const double* d_grad,
                                 const double* d_w, double rho_floor, double* d_vr, double* d_vec, double* d_sums, void* d_work,
                                 size_t work_bytes) {
    NBX_CHECK_ARG(code >= NBX_XC_SLATER && code <= NBX_XC_B3LYP5);
    return xc_functional_launch(ctx, code, 0.0, npts, d_rho, d_grad, nullptr, d_w, rho_floor, d_vr, d_vec, nullptr, d_sums, d_work,
                                work_bytes);
}

extern "C" int nbx_xc_functional_rs(nbx_ctx* ctx, int code, double omega, int64_t npts, const double* d_rho,
                                    const double* d_grad, const double* d_w, double rho_floor, double* d_vr, double* d_vec,
                                    double* d_sums, void* d_work, size_t work_bytes) {
    NBX_CHECK_ARG(code == NBX_XC_CAM_B3LYP || code == NBX_XC_LC_BLYP);
    NBX_CHECK_ARG(omega >= 0.0 && omega < 1.0e150);  // (finite; 0 is the plain B88: F(0) = 1)
    return xc_functional_launch(ctx, code, omega, npts, d_rho, d_grad, nullptr, d_w, rho_floor, d_vr, d_vec, nullptr, d_sums, d_work,
                                work_bytes);
}

extern "C" int nbx_xc_functional_mgga(nbx_ctx* ctx, int code, int64_t npts, const double* d_rho, const double* d_grad,
                                      const double* d_tau, const double* d_w, double rho_floor, double* d_vr, double* d_vec,
                                      double* d_vt, double* d_sums, void* d_work, size_t work_bytes) {
    NBX_CHECK_ARG(code == NBX_XC_TPSS || code == NBX_XC_TPSSH);
    NBX_CHECK_ARG(d_tau && d_vt);
    return xc_functional_launch(ctx, code, 0.0, npts, d_rho, d_grad, d_tau, d_w, rho_floor, d_vr, d_vec, d_vt, d_sums, d_work,
                                work_bytes);
}

extern "C" size_t nbx_xc_vmat_worksize(int64_t npts, int64_t nao) {
    if (npts <= 0 || nao <= 0) return 256;
    const int64_t nchunk = nbx_cdiv(npts, vmat_chunk(npts, nao));
    return xc_align256((size_t)(nchunk * 2 * nao * nao) * sizeof(double));
}

extern "C" size_t nbx_xc_vmat_tau_worksize(int64_t npts, int64_t nao) { return nbx_xc_vmat_worksize(npts, nao); }

namespace {

// nbx_xc_vmat (d_vt = nullptr) and nbx_xc_vmat_tau; the other arguments are checked here
int xc_vmat_launch(nbx_ctx* ctx, int64_t npts, int64_t nao, const double* d_ao, const double* d_dao, const double* d_vr,
                   const double* d_vec, const double* d_vt, double* d_vxc, void* d_work, size_t work_bytes) {
    NBX_CHECK_ARG(ctx && d_ao && d_dao && d_vr && d_vec && d_vxc && npts >= 0 && nao >= 1 && nao <= (1 << 15));
    const int64_t n2 = nao * nao;
    if (npts == 0) return nbx_memset(ctx, d_vxc, 0, (size_t)(2 * n2) * sizeof(double));
    NBX_CHECK_ARG(d_work && work_bytes >= nbx_xc_vmat_worksize(npts, nao));
    const int bt = vmat_bt(nao);
    const int64_t chunk = vmat_chunk(npts, nao), nchunk = nbx_cdiv(npts, chunk), nblk = nbx_cdiv(nao, 16 * bt);
    NBX_CHECK_ARG(nblk * nblk <= 65535 && nchunk < (1ll << 31));
    double* part = static_cast<double*>(d_work);
    const dim3 grid((unsigned)nchunk, (unsigned)(nblk * nblk), 2);
    // [bt - 1][tau]
    static const decltype(&xc_vmat_kernel<1, false>) kernels[5][2] = {{xc_vmat_kernel<1, false>, xc_vmat_kernel<1, true>},
                                                                      {xc_vmat_kernel<2, false>, xc_vmat_kernel<2, true>},
                                                                      {xc_vmat_kernel<3, false>, xc_vmat_kernel<3, true>},
                                                                      {xc_vmat_kernel<4, false>, xc_vmat_kernel<4, true>},
                                                                      {xc_vmat_kernel<5, false>, xc_vmat_kernel<5, true>}};
    hipLaunchKernelGGL(kernels[bt - 1][d_vt != nullptr], grid, dim3(64 * bt), 0, ctx->stream, npts, (int)nao, chunk, (int)nblk,
                       d_ao, d_dao, d_vr, d_vec, part, d_vt);
    NBX_LAUNCH_CHECK();
    hipLaunchKernelGGL(xc_vmat_reduce_kernel, dim3((unsigned)nbx_cdiv(2 * n2, 256)), dim3(256), 0, ctx->stream, (int)nao,
                       (int)nchunk, part, d_vxc);
    NBX_LAUNCH_CHECK();
    return NBX_OK;
}

}  // namespace

extern "C" int nbx_xc_vmat(nbx_ctx* ctx, int64_t npts, int64_t nao, const double* d_ao, const double* d_dao,
                           const double* d_vr, const double* d_vec, double* d_vxc, void* d_work, size_t work_bytes) {
    return xc_vmat_launch(ctx, npts, nao, d_ao, d_dao, d_vr, d_vec, nullptr, d_vxc, d_work, work_bytes);
}

extern "C" int nbx_xc_vmat_tau(nbx_ctx* ctx, int64_t npts, int64_t nao, const double* d_ao, const double* d_dao,
                               const double* d_vr, const double* d_vec, const double* d_vt, double* d_vxc, void* d_work,
                               size_t work_bytes) {
    NBX_CHECK_ARG(d_vt);
    return xc_vmat_launch(ctx, npts, nao, d_ao, d_dao, d_vr, d_vec, d_vt, d_vxc, d_work, work_bytes);
}
