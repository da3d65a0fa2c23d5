// Pseudo-spherical direct beam, gfx950: the beam is attenuated along its slant path through spherical
// shells, everything scattered is transported plane-parallel as before.
//
//   k_beam_slant        sigma[b][t], the slant optical depth of the beam at level t: one lane per (column, level), the O(L)
//                       sum over the shells above the level per lane (O(L^2) per column).
//   k_first_order_beam  the first order layer by layer on a beam path sigma that is an INPUT (sigma = tau / mu0 gives the
//                       coded three-zone first order of kernels.hip, which is how the kernel is pinned): one lane per
//                       (column, direction pair); a lane runs the downward recurrence of direction N-1-i, reflects it at the
//                       surface into its own mirror direction N+i and runs the upward recurrence -- no lane waits for another.
//   k_epilogue_beam     k_epilogue (epilogue.hip) with the two beam terms of the fluxes on the path sigma.
//
// The kernels read the columns as sosrt_set_columns* uploaded them (ColScalars: scalars and zone tables) and write nothing but
// their outputs.
#include "beam.hpp"
#include "stage_math.hpp"

#include "../../include/sosrt.h"

namespace sosrt {

namespace {

#define SOSRT_PI 3.14159265358979323846

// ------------------------------------------------------------------------------------------
// k_beam_slant
// sigma_t = sum_{k=1..t} (tau_k - tau_{k-1}) c_{t,k},  c_{t,k} = (r_{k-1} + r_k) / (s_{k-1} + s_k),  s_k = sqrt(r_k^2 - p^2),
// p^2 = r_t^2 (1 - mu0^2): the path through shell k over its thickness, without the cancellation of s_{k-1} - s_k.  Summed as
// (tau_t - tau_0) + sum (tau_k - tau_{k-1}) (c_{t,k} - 1) with c - 1 = (e_{k-1} + e_k) / (s_{k-1} + s_k), e_k = r_k - s_k =
// p^2 / (r_k + s_k): the plane part carries no rounding of the sum, and mu0 = 1 (p = 0) gives tau_t - tau_0 exactly.
// Every radicand is >= r_t^2 mu0^2 > 0 (levels descend, mu0 > 0).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_beam_slant(int L, int B, const double* __restrict__ tau_all, const double* __restrict__ z,
                                                   double earth_radius, const double* __restrict__ mu0_all,
                                                   double* __restrict__ sigma_all) {
    const int nblk = (L + 63) / 64;
    const int b = blockIdx.x / nblk, t0 = (blockIdx.x % nblk) * 64, t = t0 + threadIdx.x;
    if (b >= B) return;
    extern __shared__ double sm[];
    double* s_tau = sm;        // [L]
    double* s_r = sm + L;      // [L]
    const int tmax = min(L - 1, t0 + 63);                    // the shells this block's levels look through
    for (int i = threadIdx.x; i <= tmax; i += 64) {
        s_tau[i] = tau_all[(size_t)b * L + i];
        s_r[i] = earth_radius + z[i];
    }
    __syncthreads();
    if (t >= L) return;
    const double mu0 = mu0_all[b];
    const double rt = s_r[t];
    const double p2 = rt * rt * (1.0 - mu0 * mu0);
    double sp = sqrt(fmax(s_r[0] * s_r[0] - p2, 0.0));
    double ep = p2 / (s_r[0] + sp);
    double acc = 0;
    for (int k = 1; k <= t; ++k) {
        const double rk = s_r[k];
        const double sk = sqrt(fmax(rk * rk - p2, 0.0));
        const double ek = p2 / (rk + sk);
        acc += (s_tau[k] - s_tau[k - 1]) * ((ep + ek) / (sp + sk));
        sp = sk; ep = ek;
    }
    sigma_all[(size_t)b * L + t] = (s_tau[t] - s_tau[0]) + acc;
}

// ------------------------------------------------------------------------------------------
// k_first_order_beam
// With a = |mu|, Delta the optical thickness of a layer, E = e^{-Delta / a}, dsig the beam's slant thickness of the layer:
//   downward  D_t = D_{t-1} E + q_t F0 e^{-sigma_t} (Delta / a) phi(Delta / a - dsig)
//                             + [t not the first row of a zone below the top one] q_t[mirror] R e^{-(T - tau_t) / mu0} (Delta / a) phi(Delta / a + Delta / mu0)
//   surface   U_{L-1} = rho D_{L-1}[mirror]
//   upward    U_t = U_{t+1} E + q_t F0 e^{-sigma_t} (Delta / a) phi(Delta / a + dsig)
//                             + [t not the last row of a zone above the bottom one] q_t[mirror] R e^{-(T - tau_t) / mu0} (Delta / a) phi(Delta / a - Delta / mu0)
//   mu = 0    q_t F0 e^{-sigma_t} + q_t[mirror] R e^{-(T - tau_t) / mu0}
// (the reflected beam R = F0 rho e^{-sigma_{L-1} - (T - tau_{L-1}) / mu0} travels upward plane-parallel; the two exclusions are
// the reference's level choices).  A layer takes the q of the row the sweep arrives at (downward) or leaves (upward).
// The three exponentials of a row (E and the two phi) do not depend on the recurrence: kCH rows are evaluated together, and the
// dependent chain is one fused multiply-add per row.  The two beam attenuations of a row do not depend on the direction: once per
// row and workgroup, in LDS.
// ZP0: P0r_all is [B][p0z][D] and zone z of a column reads its own row (sosrt_set_aerosol_sets with a zone table).
// ------------------------------------------------------------------------------------------
constexpr int kCH = 4;

template <bool ZP0>
__global__ __launch_bounds__(64) void k_first_order_beam(Grid g, int B, ColScalars sc, const double* __restrict__ tau_all,
                                                         const double* __restrict__ sig_all, const double* __restrict__ P0a_all,
                                                         const double* __restrict__ P0r_all, int p0z, double* __restrict__ I1_all) {
    const int L = g.L, N = g.N, D = g.D;
    const int nblk = (N + 63) / 64;
    const int b = blockIdx.x / nblk, i = (blockIdx.x % nblk) * 64 + threadIdx.x;
    if (b >= B) return;
    extern __shared__ double sm[];
    double* s_tau = sm;             // [L]
    double* s_sig = s_tau + L;      // [L]
    double* s_e0 = s_sig + L;       // [L] F0 e^{-sigma_t}
    double* s_eT = s_e0 + L;        // [L] R e^{-(T - tau_t) / mu0}
    const double* tau = tau_all + (size_t)b * L;
    const double* sig = sig_all + (size_t)b * L;
    const double mu0 = sc.mu0[b], T = sc.T[b], rho = sc.rho[b], wa = sc.alb_atm[b], da = sc.dtau_atm[b];
    const double F0 = SOSRT_PI / mu0;                                        // spec:105
    const double R = F0 * rho * exp(-sig[L - 1] - (T - tau[L - 1]) / mu0);   // the reflected beam at the surface
    const double rmu0 = 1.0 / mu0;
    for (int t = threadIdx.x; t < L; t += 64) {
        const double tt = tau[t], ss = sig[t];
        s_tau[t] = tt;
        s_sig[t] = ss;
        s_e0[t] = F0 * exp(-ss);
        s_eT[t] = R * exp(-(T - tt) / mu0);
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
    const int nz = sc.nz[b];
    const int* zr0 = sc.zr0 + (size_t)b * kMaxZones;
    const int* zmix = sc.zmix + (size_t)b * kMaxZones;
    const double* zwr = sc.zwr + (size_t)b * kMaxZones;
    const double* zdtr = sc.zdtr + (size_t)b * kMaxZones;
    // q of zone z at the lane's two directions (spec:149)
    auto zone_q = [&](int z, double& q_lo, double& q_hi) {
        q_lo = wa * pa_lo * c4pi;
        q_hi = wa * pa_hi * c4pi;
        if (zmix[z]) {
            const double dr = zdtr[z], wr = zwr[z];
            const double fa = da / (da + dr), fr = dr / (da + dr);
            const double* pr = ZP0 ? P0r + (size_t)z * D : P0r;
            q_lo = (wa * pa_lo * fa + wr * pr[md] * fr) * c4pi;
            q_hi = (wa * pa_hi * fa + wr * pr[mup] * fr) * c4pi;
        }
    };

    // ---- downward, direction md ----
    double Dv = 0;
    for (int z = 0; z < nz; ++z) {
        const int r0 = zr0[z], r1 = z + 1 < nz ? zr0[z + 1] - 1 : L - 1;
        double q_lo, q_hi;
        zone_q(z, q_lo, q_hi);
        if (z == 0 && valid) I1[md] = node ? q_lo * s_e0[0] + q_hi * s_eT[0] : 0.0;          // D_0 = 0
        const bool top = z == 0;
        for (int tb = max(r0, 1); tb <= r1; tb += kCH) {
            double E[kCH], S[kCH], V[kCH];
#pragma unroll
            for (int u = 0; u < kCH; ++u) {
                const int t = min(tb + u, r1);
                const double dl = s_tau[t] - s_tau[t - 1], ds = s_sig[t] - s_sig[t - 1];
                const double x = dl * rad;
                const double e0 = s_e0[t], eT = s_eT[t];
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
        double q_lo, q_hi;
        zone_q(z, q_lo, q_hi);
        const bool bottom = z == nz - 1;
        if (bottom && valid) I1[(size_t)(L - 1) * D + mup] = node ? q_hi * s_e0[L - 1] + q_lo * s_eT[L - 1] : Uv;
        for (int tb = min(r1, L - 2); tb >= r0; tb -= kCH) {
            double E[kCH], S[kCH], V[kCH];
#pragma unroll
            for (int u = 0; u < kCH; ++u) {
                const int t = max(tb - u, r0);
                const double dl = s_tau[t + 1] - s_tau[t], ds = s_sig[t + 1] - s_sig[t];
                const double x = dl * rau;
                const double e0 = s_e0[t], eT = s_eT[t];
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
// k_epilogue_beam: k_epilogue of epilogue.hip, the same arithmetic, with the downward beam term -fb e^{-sigma_t} and the
// upward one +fb rho e^{-sigma_{L-1}} e^{-(tau_{L-1} - tau_t) / mu0}.  One workgroup per column.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_epilogue_beam(Grid g, const double* __restrict__ w_all, int B, ColScalars sc,
                                                       const double* __restrict__ tau_all, const double* __restrict__ sig_all,
                                                       const double* __restrict__ I_all, int beam_norm,
                                                       const double* __restrict__ z_profile, EpilogueOut out) {
    const int b = blockIdx.x;
    if (b >= B) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    const int L = g.L, N = g.N, D = g.D;
    extern __shared__ double s_flux[];                       // [2 L]: flux_down + flux_up with the F0/(4 pi) beam terms; heating rate
    const double* tau = tau_all + (size_t)b * L;
    const double* sig = sig_all + (size_t)b * L;
    const double mu0 = sc.mu0[b], rho = sc.rho[b];
    const double F0 = SOSRT_PI / mu0;
    const double f4 = F0 / (4 * SOSRT_PI);
    const double fb = beam_norm ? F0 : f4;
    const double tau_last = tau[L - 1];
    const double e_sfc = exp(-sig[L - 1]);
    for (int t = wave; t < L; t += nw) {
        const double* I = I_all + ((size_t)b * L + t) * D;
        double sd = 0, su = 0, den = 0;
        for (int k = lane; k < N; k += 64) {
            const double a = I[k], c = I[N + k];
            sd += g.wflux_dn[k] * a;
            su += g.wflux_up[k] * c;
            den += w_all[k] * a + w_all[N + k] * c;
        }
        sd = wsum(sd); su = wsum(su); den = wsum(den);
        if (lane == 0) {
            const double e_dn = exp(-sig[t]), e_up = e_sfc * exp(-(tau_last - tau[t]) / mu0);
            const size_t o = (size_t)b * L + t;
            if (out.flux_down) out.flux_down[o] = sd - fb * e_dn;
            if (out.flux_up) out.flux_up[o] = su + fb * rho * e_up;
            if (out.diffusivity) out.diffusivity[o] = -(sd + su) / den;
            const double fd4 = sd - f4 * e_dn, fu4 = su + f4 * rho * e_up;
            s_flux[t] = fd4 + fu4;
            if (t == 0 && out.net_toa) out.net_toa[b] = -fd4 - fu4;
        }
    }
    __syncthreads();
    if (out.heating_rate && z_profile) {
        const double k = -(1.0 / (1.225 * 1004));            // graphe:71-72
        double* s_hr = s_flux + L;                           // [L]
        for (int t = tid; t < L; t += blockDim.x) {
            const int s = t == L - 1 ? L - 2 : t;
            s_hr[t] = k * (s_flux[s + 1] - s_flux[s]) / (z_profile[s + 1] - z_profile[s]);
        }
        __syncthreads();
        const int nz = sc.nz[b];
        if (tid == 0 && nz >= 3) {
            // graphe:87-91 'erase_pics' per aerosol zone, as k_epilogue applies it
            for (int z = 1; z < nz; ++z) {
                if (!sc.zmix[(size_t)b * kMaxZones + z]) continue;
                const int iu = sc.zr0[(size_t)b * kMaxZones + z];
                const int id = z + 1 < nz ? sc.zr0[(size_t)b * kMaxZones + z + 1] - 1 : L - 1;
                auto at = [&](int i) { return i < 0 ? i + L : i; };
                s_hr[at(iu - 1)] = s_hr[at(iu - 2)];
                s_hr[at(id)] = s_hr[at(id - 1)];
            }
        }
        __syncthreads();
        double* hr = out.heating_rate + (size_t)b * L;
        for (int t = tid; t < L; t += blockDim.x) hr[t] = s_hr[t];
    }
}

}  // namespace

void launch_beam_slant(hipStream_t s, int L, int B, const double* tau, const double* z, double earth_radius, const double* mu0,
                       double* sigma) {
    const int nblk = (L + 63) / 64;
    hipLaunchKernelGGL(k_beam_slant, dim3((unsigned)B * nblk), dim3(64), (size_t)2 * L * sizeof(double), s, L, B, tau, z,
                       earth_radius, mu0, sigma);
}

void launch_first_order_beam(hipStream_t s, const Grid& g, int B, ColScalars sc, const double* tau, const double* sigma,
                             const double* P0a, const double* P0r, int p0r_zones, double* I1) {
    const int nblk = (g.N + 63) / 64;
    const size_t shm = (size_t)4 * g.L * sizeof(double);
    if (p0r_zones > 0)
        hipLaunchKernelGGL(k_first_order_beam<true>, dim3((unsigned)B * nblk), dim3(64), shm, s, g, B, sc, tau, sigma, P0a, P0r,
                           p0r_zones, I1);
    else
        hipLaunchKernelGGL(k_first_order_beam<false>, dim3((unsigned)B * nblk), dim3(64), shm, s, g, B, sc, tau, sigma, P0a, P0r,
                           0, I1);
}

void launch_epilogue_beam(hipStream_t s, const Grid& g, const double* w, int B, ColScalars sc, const double* tau,
                          const double* sigma, const double* I, int beam_norm, const double* z_profile, const EpilogueOut& out) {
    hipLaunchKernelGGL(k_epilogue_beam, dim3(B), dim3(256), (size_t)2 * g.L * sizeof(double), s, g, w, B, sc, tau, sigma, I,
                       beam_norm, z_profile, out);
}

}  // namespace sosrt
