// Per-level weights on the source function, gfx950: a pure absorber in a layer multiplies the source of its
// row by w_t = Delta tau_scattering / (Delta tau_scattering + Delta tau_gas), for both constituents alike; two weights per row,
// one on each row coefficient of the contraction, carry any per-level albedo of the atmosphere and any per-level aerosol
// fraction of a slab relative to the zone's nominal values.
//
//   k_row_weights_copy     the caller's weights into the handle's buffers (ones where a source is null), in stream order
//   k_row_weights_apply    rowcoef_a *= w_atm, rowcoef_r *= w_aer behind k_prepare: every contraction path multiplies by the
//                          coefficients row by row, so the order loop needs nothing else
//   k_first_order_profile  k_first_order_beam (beam.hip) with q of a ROW: the zone's omega times the row's weight
//   k_emission_profile     k_emission (emission.hip) with the emission coefficient of a ROW
//
// The two stage kernels are one workgroup per column like their models and keep their arithmetic: with unit weights every
// product by a weight is exact, and the expressions are the models' own (stage_math.hpp holds what the files share).  The weights of a column are loaded once, coalesced,
// into LDS (already times the zone's omega), outside the lane loop.
#include "profile.hpp"
#include "stage_math.hpp"

#include "../../include/sosrt.h"

namespace sosrt {

namespace {

#define SOSRT_PI 3.14159265358979323846

__global__ __launch_bounds__(256) void k_row_weights_copy(size_t n, size_t n_src, const double* __restrict__ src_a,
                                                          const double* __restrict__ src_r, double* __restrict__ dst_a,
                                                          double* __restrict__ dst_r) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    dst_a[i] = (src_a && i < n_src) ? src_a[i] : 1.0;
    dst_r[i] = (src_r && i < n_src) ? src_r[i] : 1.0;
}

__global__ __launch_bounds__(256) void k_row_weights_apply(size_t n, const double* __restrict__ w_atm, const double* __restrict__ w_aer,
                                                           double* __restrict__ rowcoef_a, double* __restrict__ rowcoef_r) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    rowcoef_a[i] *= w_atm[i];
    rowcoef_r[i] *= w_aer[i];
}

// ------------------------------------------------------------------------------------------
// k_first_order_profile: the recurrences, level choices, exclusions, R, phi and mu = 0 lane of k_first_order_beam, with
//   q_t[m] = (omega_atm w_atm,t P0_atm[m] f_atm + omega_aer w_aer,t P0_aer[m] f_aer) / 4 pi        (f of row t's zone; clear: f_atm = 1)
// s_wa[t] = omega_atm w_atm,t and s_wr[t] = omega_aer(zone of t) w_aer,t are formed once per row and workgroup.
// ------------------------------------------------------------------------------------------
constexpr int kCH = 4;

template <bool ZP0>
__global__ __launch_bounds__(64) void k_first_order_profile(Grid g, int B, ColScalars sc, const double* __restrict__ tau_all,
                                                            const double* __restrict__ sig_all, const double* __restrict__ P0a_all,
                                                            const double* __restrict__ P0r_all, int p0z,
                                                            const double* __restrict__ wa_all, const double* __restrict__ wr_all,
                                                            double* __restrict__ I1_all) {
    const int L = g.L, N = g.N, D = g.D;
    const int nblk = (N + 63) / 64;
    const int b = blockIdx.x / nblk, i = (blockIdx.x % nblk) * 64 + threadIdx.x;
    if (b >= B) return;
    extern __shared__ double sm[];
    double* s_tau = sm;             // [L]
    double* s_sig = s_tau + L;      // [L]
    double* s_e0 = s_sig + L;       // [L] F0 e^{-sigma_t}
    double* s_eT = s_e0 + L;        // [L] R e^{-(T - tau_t) / mu0}
    double* s_wa = s_eT + L;        // [L] omega_atm w_atm,t
    double* s_wr = s_wa + L;        // [L] omega_aer of the row's zone times w_aer,t (0 in a clear zone)
    const double* tau = tau_all + (size_t)b * L;
    const double* sig = sig_all + (size_t)b * L;
    const double mu0 = sc.mu0[b], T = sc.T[b], rho = sc.rho[b], wa = sc.alb_atm[b], da = sc.dtau_atm[b];
    const double F0 = SOSRT_PI / mu0;                                        // spec:105
    const double R = F0 * rho * exp(-sig[L - 1] - (T - tau[L - 1]) / mu0);   // the reflected beam at the surface
    const double rmu0 = 1.0 / mu0;
    const int nz = sc.nz[b];
    // the column's zone table, once per workgroup: first rows, kinds and the fractions of spec:149 (the sweeps index it by zone)
    __shared__ int zr0[kMaxZones], zmix[kMaxZones];
    __shared__ double zwr[kMaxZones], s_zfa[kMaxZones], s_zfr[kMaxZones];
    if (threadIdx.x < kMaxZones) {
        const int z = threadIdx.x;
        const bool in = z < nz;
        const double dr = in ? sc.zdtr[(size_t)b * kMaxZones + z] : 0.0;
        zr0[z] = in ? sc.zr0[(size_t)b * kMaxZones + z] : L;
        zmix[z] = in ? sc.zmix[(size_t)b * kMaxZones + z] : 0;
        zwr[z] = in ? sc.zwr[(size_t)b * kMaxZones + z] : 0.0;
        s_zfa[z] = da / (da + dr);
        s_zfr[z] = dr / (da + dr);
    }
    __syncthreads();
    for (int t = threadIdx.x; t < L; t += 64) {
        const double tt = tau[t], ss = sig[t];
        const int z = zone_of(zr0, nz, t);
        s_tau[t] = tt;
        s_sig[t] = ss;
        s_e0[t] = F0 * exp(-ss);
        s_eT[t] = R * exp(-(T - tt) / mu0);
        s_wa[t] = wa * wa_all[(size_t)b * L + t];
        s_wr[t] = zmix[z] ? zwr[z] * wr_all[(size_t)b * L + t] : 0.0;
    }
    __syncthreads();
    const bool valid = i < N;
    const int ii = valid ? i : 0;
    const int md = N - 1 - ii, mup = N + ii;                 // the lane's downward direction and its mirror, the upward one
    const bool node = ii == 0;                               // the two mu = 0 nodes
    const double ad = node ? 1.0 : -g.mu[md], au = node ? 1.0 : g.mu[mup];
    const double rad = 1.0 / ad, rau = 1.0 / au;
    const double c4pi = 1.0 / (4 * SOSRT_PI);
    const double* P0a = P0a_all + (size_t)b * D;
    const double* P0r = P0r_all + (size_t)b * (ZP0 ? p0z : 1) * D;
    const double pa_lo = P0a[md], pa_hi = P0a[mup];
    double* I1 = I1_all + (size_t)b * L * D;
    // what q of a row of zone z needs besides the row's two weighted albedos: the zone's fractions and its aerosol P0
    bool zmx = false;
    double zfa = 1.0, zfr = 0.0, zp_lo = 0.0, zp_hi = 0.0;
    auto zone_q = [&](int z) {
        zmx = zmix[z] != 0;
        if (zmx) {
            zfa = s_zfa[z]; zfr = s_zfr[z];
            const double* pr = ZP0 ? P0r + (size_t)z * D : P0r;
            zp_lo = pr[md]; zp_hi = pr[mup];
        }
    };
    auto row_q = [&](int t, double& q_lo, double& q_hi) {
        const double wat = s_wa[t];
        q_lo = wat * pa_lo * c4pi;
        q_hi = wat * pa_hi * c4pi;
        if (zmx) {
            const double wrt = s_wr[t];
            q_lo = (wat * pa_lo * zfa + wrt * zp_lo * zfr) * c4pi;
            q_hi = (wat * pa_hi * zfa + wrt * zp_hi * zfr) * c4pi;
        }
    };

    // ---- downward, direction md ----
    double Dv = 0;
    for (int z = 0; z < nz; ++z) {
        const int r0 = zr0[z], r1 = z + 1 < nz ? zr0[z + 1] - 1 : L - 1;
        zone_q(z);
        if (z == 0 && valid) {
            double q_lo, q_hi;
            row_q(0, q_lo, q_hi);
            I1[md] = node ? q_lo * s_e0[0] + q_hi * s_eT[0] : 0.0;          // D_0 = 0
        }
        const bool top = z == 0;
        for (int tb = max(r0, 1); tb <= r1; tb += kCH) {
            double E[kCH], S[kCH], V[kCH];
#pragma unroll
            for (int u = 0; u < kCH; ++u) {
                const int t = min(tb + u, r1);
                const double dl = s_tau[t] - s_tau[t - 1], ds = s_sig[t] - s_sig[t - 1];
                const double x = dl * rad;
                const double e0 = s_e0[t], eT = s_eT[t];
                double q_lo, q_hi;
                row_q(t, q_lo, q_hi);
                E[u] = exp(-x);
                const double direct = q_lo * e0 * x * phi1(x - ds);
                const double refl = q_hi * eT * x * phi1(x + dl * rmu0);
                S[u] = (top || t != r0) ? direct + refl : direct;
                V[u] = q_lo * e0 + q_hi * eT;
            }
#pragma unroll
            for (int u = 0; u < kCH; ++u) {
                const int t = tb + u;
                if (t <= r1) {
                    Dv = fma(Dv, E[u], S[u]);
                    if (valid) I1[(size_t)t * D + md] = node ? V[u] : Dv;
                }
            }
        }
    }
    // ---- surface and upward, direction mup (its mirror is md: the lane's own downward value) ----
    double Uv = rho * Dv;
    for (int z = nz - 1; z >= 0; --z) {
        const int r0 = zr0[z], r1 = z + 1 < nz ? zr0[z + 1] - 1 : L - 1;
        zone_q(z);
        const bool bottom = z == nz - 1;
        if (bottom && valid) {
            double q_lo, q_hi;
            row_q(L - 1, q_lo, q_hi);
            I1[(size_t)(L - 1) * D + mup] = node ? q_hi * s_e0[L - 1] + q_lo * s_eT[L - 1] : Uv;
        }
        for (int tb = min(r1, L - 2); tb >= r0; tb -= kCH) {
            double E[kCH], S[kCH], V[kCH];
#pragma unroll
            for (int u = 0; u < kCH; ++u) {
                const int t = max(tb - u, r0);
                const double dl = s_tau[t + 1] - s_tau[t], ds = s_sig[t + 1] - s_sig[t];
                const double x = dl * rau;
                const double e0 = s_e0[t], eT = s_eT[t];
                double q_lo, q_hi;
                row_q(t, q_lo, q_hi);
                E[u] = exp(-x);
                const double direct = q_hi * e0 * x * phi1(x + ds);
                const double refl = q_lo * eT * x * phi1(x - dl * rmu0);
                S[u] = (bottom || t != r1) ? direct + refl : direct;
                V[u] = q_hi * e0 + q_lo * eT;
            }
#pragma unroll
            for (int u = 0; u < kCH; ++u) {
                const int t = tb - u;
                if (t >= r0) {
                    Uv = fma(Uv, E[u], S[u]);
                    if (valid) I1[(size_t)t * D + mup] = node ? V[u] : Uv;
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// k_emission_profile: the sweeps and the boundary of k_emission with the emission coefficient of a ROW,
//   eps_t = 1 - (omega_atm w_atm,t f_atm + omega_aer w_aer,t f_aer)        (f of row t's zone; clear: 1 - omega_atm w_atm,t)
// formed once per row and workgroup in LDS.  The layer between rows t-1 and t takes eps_t in BOTH sweeps, as there; with eps a
// row's, the zones are no loop of the sweeps any more: rows 1 .. L-1 in chunks of kCH.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_emission_profile(Grid g, int B, ColScalars sc, int surface, const double* __restrict__ tau_all,
                                                           const double* __restrict__ pl_all, const double* __restrict__ bs_all,
                                                           const double* __restrict__ es_all, const double* __restrict__ wa_all,
                                                           const double* __restrict__ wr_all, double* __restrict__ I0_all) {
    const int L = g.L, N = g.N, D = g.D;
    const int b = blockIdx.x, i = threadIdx.x;
    if (b >= B) return;                                      // (uniform over the workgroup)
    extern __shared__ double sm[];
    double* s_tau = sm;             // [L]
    double* s_b = s_tau + L;        // [L]
    double* s_eps = s_b + L;        // [L] emission coefficient of the row
    double* s_sfc = s_eps + L;      // [N] the downward surface row (Lambertian grounds)
    double* s_red = s_sfc + N;      // [16]
    const double* tau = tau_all + (size_t)b * L;
    const double* pl = pl_all + (size_t)b * L;
    {
        const double wa = sc.alb_atm[b], da = sc.dtau_atm[b];
        const int nz = sc.nz[b];
        const int* zr0 = sc.zr0 + (size_t)b * kMaxZones;
        for (int t = i; t < L; t += blockDim.x) {
            s_tau[t] = tau[t];
            s_b[t] = pl[t];
            const int z = zone_of(zr0, nz, t);
            const double wat = wa * wa_all[(size_t)b * L + t];
            double eps = 1.0 - wat;
            if (sc.zmix[(size_t)b * kMaxZones + z]) {
                const double dr = sc.zdtr[(size_t)b * kMaxZones + z];
                const double wrt = sc.zwr[(size_t)b * kMaxZones + z] * wr_all[(size_t)b * L + t];
                eps = 1.0 - (wat * (da / (da + dr)) + wrt * (dr / (da + dr)));
            }
            s_eps[t] = eps;
        }
    }
    __syncthreads();
    const double rho = sc.rho[b];
    const double ground = (es_all ? es_all[b] : 1.0 - rho) * bs_all[b];
    const bool valid = i < N;
    const int ii = valid ? i : 0;
    const int md = N - 1 - ii, mup = N + ii;                 // the lane's downward direction and its mirror, the upward one
    const bool node = ii == 0;                               // the two mu = 0 nodes
    const double rad = node ? 1.0 : -1.0 / g.mu[md], rau = node ? 1.0 : 1.0 / g.mu[mup];
    double* I0 = I0_all + (size_t)b * L * D;

    // ---- downward, direction md; the node lane writes eps_t b_t to both nodes of a row ----
    double Dv = 0;
    if (valid) {
        I0[md] = node ? s_eps[0] * s_b[0] : 0.0;             // D_0 = 0
        if (node) I0[mup] = s_eps[0] * s_b[0];
    }
    for (int tb = 1; tb <= L - 1; tb += kCH) {
        double E[kCH], S[kCH], V[kCH];
#pragma unroll
        for (int u = 0; u < kCH; ++u) {
            const int t = min(tb + u, L - 1);
            const double x = (s_tau[t] - s_tau[t - 1]) * rad;
            const double bc = s_b[t], bp = s_b[t - 1], eps = s_eps[t];
            double w0, w1;
            E[u] = exp(-x);
            linear_weights(x, E[u], w0, w1);
            S[u] = eps * (w0 * bc + w1 * bp);
            V[u] = eps * bc;
        }
#pragma unroll
        for (int u = 0; u < kCH; ++u) {
            const int t = tb + u;
            if (t <= L - 1) {
                Dv = fma(Dv, E[u], S[u]);
                if (valid) {
                    I0[(size_t)t * D + md] = node ? V[u] : Dv;
                    if (node) I0[(size_t)t * D + mup] = V[u];
                }
            }
        }
    }
    // ---- ground: the order loop's rule for the handle's surface, as k_emission applies it ----
    double Bv = 0;
    if (surface == SOSRT_SURFACE_SPECULAR) {
        Bv = rho * Dv;                                       // the mirror lane: the lane's own downward value
    } else if (surface == SOSRT_SURFACE_LAMBERTIAN || surface == SOSRT_SURFACE_LAMBERTIAN_README) {
        if (valid) s_sfc[md] = Dv;
        __syncthreads();
        double term = 0;
        if (i <= N - 3) {
            const int k0 = N - 2 - i, k1 = N - 3 - i;
            const double x0 = g.mu[k0], x1 = g.mu[k1];
            term = (x1 - x0) * (s_sfc[k1] * x1 + s_sfc[k0] * x0) / 2;
        }
        const double v = wsum(term);
        if ((i & 63) == 0) s_red[i >> 6] = v;
        __syncthreads();
        double S = 0;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) S += s_red[w];
        Bv = (surface == SOSRT_SURFACE_LAMBERTIAN_README ? 2 : -2) * rho * S;
    }
    // ---- upward, direction mup ----
    double Uv = Bv + ground;
    if (valid && !node) I0[(size_t)(L - 1) * D + mup] = Uv;
    for (int tb = L - 1; tb >= 1; tb -= kCH) {               // tb: the row the sweep leaves; it arrives at tb - 1
        double E[kCH], S[kCH];
#pragma unroll
        for (int u = 0; u < kCH; ++u) {
            const int t1 = max(tb - u, 1);
            const double x = (s_tau[t1] - s_tau[t1 - 1]) * rau;
            const double bc = s_b[t1 - 1], bp = s_b[t1], eps = s_eps[t1];
            double w0, w1;
            E[u] = exp(-x);
            linear_weights(x, E[u], w0, w1);
            S[u] = eps * (w0 * bc + w1 * bp);
        }
#pragma unroll
        for (int u = 0; u < kCH; ++u) {
            const int t1 = tb - u;
            if (t1 >= 1) {
                Uv = fma(Uv, E[u], S[u]);
                if (valid && !node) I0[(size_t)(t1 - 1) * D + mup] = Uv;
            }
        }
    }
}

}  // namespace

void launch_row_weights_copy(hipStream_t s, size_t n, size_t n_src, const double* src_a, const double* src_r, double* dst_a,
                             double* dst_r) {
    hipLaunchKernelGGL(k_row_weights_copy, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, n_src, src_a, src_r, dst_a, dst_r);
}

void launch_row_weights_apply(hipStream_t s, size_t n, const double* w_atm, const double* w_aer, double* rowcoef_a, double* rowcoef_r) {
    hipLaunchKernelGGL(k_row_weights_apply, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, w_atm, w_aer, rowcoef_a, rowcoef_r);
}

void launch_first_order_profile(hipStream_t s, const Grid& g, int B, ColScalars sc, const double* tau, const double* sigma,
                                const double* P0a, const double* P0r, int p0r_zones, const double* w_atm, const double* w_aer,
                                double* I1) {
    const int nblk = (g.N + 63) / 64;
    const size_t shm = (size_t)6 * g.L * sizeof(double);
    if (p0r_zones > 0)
        hipLaunchKernelGGL(k_first_order_profile<true>, dim3((unsigned)B * nblk), dim3(64), shm, s, g, B, sc, tau, sigma, P0a, P0r,
                           p0r_zones, w_atm, w_aer, I1);
    else
        hipLaunchKernelGGL(k_first_order_profile<false>, dim3((unsigned)B * nblk), dim3(64), shm, s, g, B, sc, tau, sigma, P0a, P0r,
                           0, w_atm, w_aer, I1);
}

void launch_emission_profile(hipStream_t s, const Grid& g, int B, ColScalars sc, int surface, const double* tau, const double* planck,
                             const double* planck_surface, const double* emissivity, const double* w_atm, const double* w_aer,
                             double* I0) {
    const int threads = (g.N + 63) / 64 * 64;
    const size_t shm = ((size_t)3 * g.L + g.N + 16) * sizeof(double);
    hipLaunchKernelGGL(k_emission_profile, dim3((unsigned)B), dim3(threads), shm, s, g, B, sc, surface, tau, planck, planck_surface,
                       emissivity, w_atm, w_aer, I0);
}

}  // namespace sosrt
