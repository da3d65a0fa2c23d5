// Kernels either side of the order loop, gfx950:
//
//   k_epilogue      what the reference's callers consume from a converged field, computed where the field
//                   lives: downward / upward flux per level (graphe:157-158, crit:380-381), diffusivity
//                   (graphe:10), heating rate incl. the 'erase_pics' fix-up (graphe:74-91; at every aerosol
//                   zone of the column's zone table) and the net flux
//                   at the top of the atmosphere (crit:382).  One workgroup per column, one wavefront per
//                   layer row at a time (a row of 2N doubles is read once, coalesced); the per-level net
//                   flux stays in LDS for the finite differences of the heating rate.
//   k_azimuth_accumulate / k_view_azimuth_accumulate / k_azimuth_synthesize
//                   synthesis I(phi) = sum_m (2 - delta_m0) I^m cos(m phi) on the requested levels.
//   k_mie_coefficients / k_mie_angles / k_mie_integrate
//                   the table p(cos Theta) of a Mie sphere or of a log-normal ensemble of them (phase:299, 398-489; the
//                   series of sosrt/mie.py), with the ensemble's single-scattering albedo and asymmetry parameter
//                   (DESIGN section 12): a_n, b_n and the efficiencies with one lane per (ensemble, radius), the angular
//                   sums with one lane per table abscissa and a_n, b_n as wave-uniform loads, then the trapezoid over radii.
//
// The builders of the phase matrix, of P0 and of their Fourier modes are in phase.hip.
#include "kernels.hpp"

#include "../../include/sosrt.h"

namespace sosrt {

namespace {

#define SOSRT_PI 3.14159265358979323846

__device__ __forceinline__ double wsum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(256) void k_epilogue(Grid g, const double* __restrict__ w_all, int B,
                                                  const double* __restrict__ tau_all, const double* __restrict__ I_all,
                                                  const ColDesc* __restrict__ desc, int beam_norm,
                                                  const double* __restrict__ z_profile, EpilogueOut out) {
    const int b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    const int L = g.L, N = g.N, D = g.D;
    extern __shared__ double s_flux[];                       // [2 L]: flux_down + flux_up with the F0/(4 pi) beam terms; heating rate
    const ColDesc& d = desc[b];
    const double* tau = tau_all + (size_t)b * L;
    const double mu0 = d.mu0, rho = d.rho;
    const double F0 = SOSRT_PI / mu0;                        // spec:105
    const double f4 = F0 / (4 * SOSRT_PI);
    const double fb = beam_norm ? F0 : f4;
    const double tau_last = tau[L - 1];
    for (int t = wave; t < L; t += nw) {
        const double* I = I_all + ((size_t)b * L + t) * D;
        double sd = 0, su = 0, den = 0;
        for (int k = lane; k < N; k += 64) {
            const double a = I[k], c = I[N + k];
            sd += g.wflux_dn[k] * a;                         // trapz(I[:N] mu[:N], mu[:N])
            su += g.wflux_up[k] * c;
            den += w_all[k] * a + w_all[N + k] * c;          // trapz(I, mu) over the whole grid (graphe:10)
        }
        sd = wsum(sd); su = wsum(su); den = wsum(den);
        if (lane == 0) {
            const double e_dn = exp(-tau[t] / mu0), e_up = exp(-(2 * tau_last - tau[t]) / mu0);
            const size_t o = (size_t)b * L + t;
            if (out.flux_down) out.flux_down[o] = sd - fb * e_dn;
            if (out.flux_up) out.flux_up[o] = su + fb * rho * e_up;
            // the zero-width interval between the two mu = 0 nodes adds nothing: trapz(I mu, mu) = sd + su
            if (out.diffusivity) out.diffusivity[o] = -(sd + su) / den;
            const double fd4 = sd - f4 * e_dn, fu4 = su + f4 * rho * e_up;
            s_flux[t] = fd4 + fu4;
            if (t == 0 && out.net_toa) out.net_toa[b] = -fd4 - fu4;          // crit:382
        }
    }
    __syncthreads();
    if (out.heating_rate && z_profile) {
        const double k = -(1.0 / (1.225 * 1004));            // graphe:71-72: -(1 / (rho c_p))
        double* s_hr = s_flux + L;                           // [L]
        // graphe:83-85: forward difference, the last level copies the one above
        for (int t = tid; t < L; t += blockDim.x) {
            const int s = t == L - 1 ? L - 2 : t;
            s_hr[t] = k * (s_flux[s + 1] - s_flux[s]) / (z_profile[s + 1] - z_profile[s]);
        }
        __syncthreads();
        if (tid == 0 && d.nz >= 3) {
            // graphe:87-91 'erase_pics', per aerosol zone, in the reference's statement order (Python indexing: -1 is the
            // last level): the level above a slab and the slab's last level take the value of their upper neighbour
            for (int z = 1; z < d.nz; ++z) {
                if (!d.mix[z]) continue;
                const int iu = d.r0[z], id = d.r1[z];
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

// one term of the synthesis, sum_m (2 - delta_m0) I^m cos(m phi): both kernels below add it, in ascending m
__device__ __forceinline__ double azimuth_term(double acc, double v, int m, double phi) { return acc + 2 * v * cos(m * phi); }

// out[b][lev][dir][j]: mode 0 writes I^0 itself, modes m >= 1 add 2 I^m cos(m phi_j).  One workgroup per (column, level);
// a level outside [0, L) gives NaN rows instead of a read out of bounds.
__global__ __launch_bounds__(256) void k_azimuth_accumulate(int L, int D, int m, const double* __restrict__ Im, int nlev,
                                                            const int* __restrict__ levels, int nphi, const double* __restrict__ phi,
                                                            double* __restrict__ out) {
    const int b = blockIdx.x / nlev, lev = blockIdx.x % nlev;
    const int t = levels[lev];
    const bool ok = t >= 0 && t < L;
    const double* row = Im + ((size_t)b * L + (ok ? t : 0)) * D;
    double* o = out + (size_t)blockIdx.x * D * nphi;
    const int n = D * nphi;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int dir = i / nphi, j = i - dir * nphi;
        const double v = ok ? row[dir] : __builtin_nan("");
        if (m == 0) o[i] = v;
        else o[i] = azimuth_term(o[i], v, m, phi[j]);
    }
}

// The same term at the view lanes: val [n] = [B][nlev][2V] is mode m of the view radiance at the requested
// levels already, out [n][nphi].  One thread per element of out.
__global__ __launch_bounds__(256) void k_view_azimuth_accumulate(size_t n, int m, const double* __restrict__ val, int nphi,
                                                                 const double* __restrict__ phi, double* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * nphi) return;
    const size_t e = i / nphi;
    const int j = (int)(i - e * nphi);
    const double v = val[e];
    if (m == 0) out[i] = v;
    else out[i] = azimuth_term(out[i], v, m, phi[j]);
}

// The same sum over all modes in one launch: I0 [B][L][D] is mode 0, Im [M][B][L][D] the modes 1..M; `out` is written once
// instead of read and rewritten per mode.  The terms are added in ascending m: the bits of the sequence of launches above.
__global__ __launch_bounds__(256) void k_azimuth_synthesize(int B, int L, int D, int M, const double* __restrict__ I0,
                                                            const double* __restrict__ Im, int nlev,
                                                            const int* __restrict__ levels, int nphi,
                                                            const double* __restrict__ phi, double* __restrict__ out) {
    const int b = blockIdx.x / nlev, lev = blockIdx.x % nlev;
    const int t = levels[lev];
    const bool ok = t >= 0 && t < L;
    const size_t ro = ((size_t)b * L + (ok ? t : 0)) * D, BLD = (size_t)B * L * D;
    double* o = out + (size_t)blockIdx.x * D * nphi;
    const int n = D * nphi;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int dir = i / nphi, j = i - dir * nphi;
        const double ph = phi[j];
        double acc = ok ? I0[ro + dir] : __builtin_nan("");
        for (int m = 1; m <= M; ++m) {
            const double v = ok ? Im[(size_t)(m - 1) * BLD + ro + dir] : __builtin_nan("");
            acc = azimuth_term(acc, v, m, ph);
        }
        o[i] = acc;
    }
}

// ---------------------------------------------------------------------------------------------
// Lorenz-Mie series and the log-normal ensemble (sosrt/mie.py; Bohren & Huffman 1983 ch. 4)
// ---------------------------------------------------------------------------------------------
struct Cx {
    double re, im;
};
// The coefficient kernel keeps products and sums apart (no contraction into FMA) and divides where the host series divides: a
// relative 1e-16 that enters every D_n or a_n alike acts like a shift of x, which the ripple structure of the efficiencies
// magnifies by ~x (x = 2000, measured on the device: 3.5e-15 from the extended-precision value with n * (1 / mx) in place of
// n / mx; the host series is 1.8e-16 from it).
__device__ __forceinline__ Cx cmul(Cx a, Cx b) {
#pragma clang fp contract(off)
    return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re};
}
// Smith's division, as NumPy divides complex128
__device__ __forceinline__ Cx cdiv(Cx a, Cx b) {
#pragma clang fp contract(off)
    if (fabs(b.re) >= fabs(b.im)) {
        const double rat = b.im / b.re, scl = 1.0 / (b.re + b.im * rat);
        return {(a.re + a.im * rat) * scl, (a.im - a.re * rat) * scl};
    }
    const double rat = b.re / b.im, scl = 1.0 / (b.im + b.re * rat);
    return {(a.re * rat + a.im) * scl, (a.im * rat - a.re) * scl};
}

// The same with two true divisions in place of the reciprocal: how the host series' n / mx rounds (a Python complex quotient)
__device__ __forceinline__ Cx cdiv_true(Cx a, Cx b) {
#pragma clang fp contract(off)
    if (fabs(b.re) >= fabs(b.im)) {
        const double rat = b.im / b.re, den = b.re + b.im * rat;
        return {(a.re + a.im * rat) / den, (a.im - a.re * rat) / den};
    }
    const double rat = b.re / b.im, den = b.re * rat + b.im;
    return {(a.re * rat + a.im) / den, (a.im * rat - a.re) / den};
}

// Compensated (Kahan) sum: the efficiencies at x = 2000 are sums of 2052 terms, and the host's pairwise sums are good to an ulp
struct Ksum {
    double s = 0, c = 0;
    __device__ __forceinline__ void add(double v) {
#pragma clang fp contract(off)
        const double y = v - c, t = s + y;
        c = (t - s) - y;
        s = t;
    }
};

// One lane per sphere (ensemble s = lane / R, radius i = lane % R): the logarithmic derivative D_n(mx) downward from nstart,
// psi_n, chi_n upward, a_n, b_n (B&H 4.88) and the sums of the efficiencies (mie.mie_coefficients, mie.efficiencies).
// ab [nlanes][n_cap][4]: row n - 1 of a lane first holds D_n (written on the way down, read once on the way up), then
// (a_n, b_n) (2n + 1) / (n (n + 1)).  qw [nlanes][kMieQ] = {Q_ext, Q_sca, Q_back, g, n(r), weight of the sphere's angular sum
// in the table}; radii == nullptr (sosrt_mie_efficiencies) leaves the last two out.  Trip counts differ between lanes; the lanes of
// a wave are neighbouring radii, whose counts are close.
__global__ __launch_bounds__(64) void k_mie_coefficients(int nlanes, int R, int n_cap, const double* __restrict__ x_all,
                                                         const int* __restrict__ nmax_all, const int* __restrict__ nstart_all,
                                                         const double* __restrict__ m_re, const double* __restrict__ m_im,
                                                         const double* __restrict__ radii, const double* __restrict__ r_m,
                                                         const double* __restrict__ sig, double* __restrict__ ab,
                                                         double* __restrict__ qw) {
#pragma clang fp contract(off)
    const int lane = blockIdx.x * blockDim.x + threadIdx.x;
    if (lane >= nlanes) return;
    const int s = lane / R, i = lane - s * R;
    const double x = x_all[lane];
    const int nmax = min(nmax_all[lane], n_cap), nstart = nstart_all[lane];
    const Cx m = {m_re[s], m_im[s]}, mx = {m.re * x, m.im * x};
    double* rec = ab + (size_t)lane * n_cap * 4;
    Cx D = {0.0, 0.0};
    for (int n = nstart; n >= 1; --n) {                      // D_{n-1} = n / mx - 1 / (D_n + n / mx)
        if (n <= nmax) { rec[(size_t)(n - 1) * 4] = D.re; rec[(size_t)(n - 1) * 4 + 1] = D.im; }
        const Cx nm = cdiv_true({(double)n, 0.0}, mx);
        const Cx q = cdiv({1.0, 0.0}, {D.re + nm.re, D.im + nm.im});
        D = {nm.re - q.re, nm.im - q.im};
    }
    double sn, cs;
    sincos(x, &sn, &cs);
    double psi0 = cs, psi1 = sn, chi0 = -sn, chi1 = cs;
    Ksum s_ext, s_sca, s_g1, s_g2;
    double sign = -1.0;
    Cx s_back = {0, 0}, a0 = {0, 0}, b0 = {0, 0};
    Cx Dn = {rec[0], rec[1]};
    for (int n = 1; n <= nmax; ++n) {
        Cx Dnext = {0, 0};
        if (n < nmax) Dnext = {rec[(size_t)n * 4], rec[(size_t)n * 4 + 1]};     // (a sweep ahead of its use: the divisions below cover the load)
        const double c = (2.0 * n - 1.0) / x, nx = n / x;
        const double psi = c * psi1 - psi0, chi = c * chi1 - chi0;
        const Cx xi = {psi, -chi}, xi1 = {psi1, -chi1};
        Cx da = cdiv(Dn, m), db = cmul(Dn, m);
        da.re += nx;
        db.re += nx;
        const Cx ta = cmul(da, xi), tb = cmul(db, xi);
        const Cx a = cdiv({da.re * psi - psi1, da.im * psi}, {ta.re - xi1.re, ta.im - xi1.im});
        const Cx b = cdiv({db.re * psi - psi1, db.im * psi}, {tb.re - xi1.re, tb.im - xi1.im});
        const double t2 = 2.0 * n + 1.0;
        s_ext.add(t2 * (a.re + b.re));
        s_sca.add(t2 * (a.re * a.re + a.im * a.im + b.re * b.re + b.im * b.im));
        s_back.re += t2 * sign * (a.re - b.re);
        s_back.im += t2 * sign * (a.im - b.im);
        const double f = t2 / ((double)n * (n + 1.0));
        s_g2.add(f * (a.re * b.re + a.im * b.im));
        if (n > 1) s_g1.add((n - 1.0) * (n + 1.0) / (double)n * (a0.re * a.re + a0.im * a.im + b0.re * b.re + b0.im * b.im));
        double* o = rec + (size_t)(n - 1) * 4;
        o[0] = f * a.re; o[1] = f * a.im; o[2] = f * b.re; o[3] = f * b.im;
        a0 = a; b0 = b; sign = -sign;
        psi0 = psi1; psi1 = psi; chi0 = chi1; chi1 = chi;
        Dn = Dnext;
    }
    const double x2 = x * x;
    const double qext = 2.0 / x2 * s_ext.s, qsca = 2.0 / x2 * s_sca.s;
    double* q = qw + (size_t)lane * kMieQ;
    q[0] = qext;
    q[1] = qsca;
    q[2] = (s_back.re * s_back.re + s_back.im * s_back.im) / x2;
    q[3] = 4.0 / (qsca * x2) * (s_g1.s + s_g2.s);
    if (radii) {
        // mie.log_normal_bulk_phase: n(r) = exp(-(ln r - ln r_m)^2 / (2 ln^2 sig)) / r, weight n(r) Q_sca(r), trapezoid over
        // r; the sphere's intensity is (|S1|^2 + |S2|^2) / (2 pi x^2 Q_ext) (mie.i_unpolarized).  One sphere: no weights.
        double nr = 1.0, w = 1.0;
        if (R > 1) {
            const double r = radii[i], dl = log(r) - log(r_m[s]), ls = log(sig[s]);
            nr = (1.0 / r) * exp(-(dl * dl) / (2 * ls * ls));
            const double lo = i > 0 ? r - radii[i - 1] : 0.0, hi = i < R - 1 ? radii[i + 1] - r : 0.0;
            w = 0.5 * (lo + hi) * nr * qsca;
        }
        q[4] = nr;
        q[5] = w / (2.0 * (SOSRT_PI * x2 * qext));
    }
}

// One lane per table abscissa mu_j, one workgroup per (block of 256 abscissae, chunk of kMieChunk radii, ensemble): the
// pi_n / tau_n recurrence of mie.amplitudes, S1 and S2, and the chunk's share of the trapezoid over radii.  The coefficients
// and (n + 1) / n are addressed by block coordinates and the loop counter only: wave-uniform loads into scalar registers.
//   pi_{n+1} = s + (n + 1) / n (s - pi_{n-1}),  tau_n = n (s - pi_{n-1}) - pi_{n-1},  s = mu pi_n
__global__ __launch_bounds__(256) void k_mie_angles(int R, int ntab, int n_cap, const double* __restrict__ mu,
                                                    const double* __restrict__ ab, const int* __restrict__ nmax_all,
                                                    const double* __restrict__ tn, const double* __restrict__ qw,
                                                    double* __restrict__ part) {
    const int j = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y, s = blockIdx.z;
    const double m = mu[min(j, ntab - 1)];
    const int i0 = c * kMieChunk, i1 = min(R, i0 + kMieChunk);
    double acc = 0;
    for (int i = i0; i < i1; ++i) {
        const int lane = s * R + i;
        const int nmax = min(nmax_all[lane], n_cap);
        const double* __restrict__ rec = ab + (size_t)lane * n_cap * 4;
        double pi0 = 0, pi1 = 1, dn = 1, s1r = 0, s1i = 0, s2r = 0, s2i = 0;
#pragma unroll 4
        for (int n = 1; n <= nmax; ++n) {
            const double ar = rec[0], ai = rec[1], br = rec[2], bi = rec[3], t = tn[n];
            rec += 4;
            const double sp = m * pi1, d = sp - pi0;
            const double tau = dn * d - pi0;
            s1r += ar * pi1 + br * tau;
            s1i += ai * pi1 + bi * tau;
            s2r += ar * tau + br * pi1;
            s2i += ai * tau + bi * pi1;
            pi0 = pi1;
            pi1 = sp + t * d;
            dn += 1.0;
        }
        acc += qw[(size_t)lane * kMieQ + 5] * (s1r * s1r + s1i * s1i + s2r * s2r + s2i * s2i);
    }
    if (j < ntab) part[((size_t)s * gridDim.y + c) * ntab + j] = acc;
}

// p[s][j] = sum of the chunks' shares in ascending order (no atomics: the same bits on every call); the workgroup behind
// the last block of abscissae reduces the ensemble's bulk numbers with the same trapezoid:
//   bulk[s] = {omega = int n r^2 Q_sca / int n r^2 Q_ext, g = int n r^2 Q_sca g / int n r^2 Q_sca,
//              mean extinction cross-section pi int n r^2 Q_ext / int n}  (one sphere: Q_sca / Q_ext, g, pi r^2 Q_ext)
__global__ __launch_bounds__(256) void k_mie_integrate(int R, int ntab, int nchunk, const double* __restrict__ part,
                                                       const double* __restrict__ radii, const double* __restrict__ qw,
                                                       double* __restrict__ p, double* __restrict__ bulk) {
    const int s = blockIdx.y;
    if (blockIdx.x == gridDim.x - 1) {
        if (threadIdx.x != 0 || !bulk) return;
        const double* q = qw + (size_t)s * R * kMieQ;
        double* o = bulk + (size_t)s * 3;
        if (R == 1) {
            o[0] = q[1] / q[0]; o[1] = q[3]; o[2] = SOSRT_PI * radii[0] * radii[0] * q[0];
            return;
        }
        double ie = 0, is = 0, ig = 0, in = 0;
        for (int i = 0; i + 1 < R; ++i) {
            const double r0 = radii[i], r1 = radii[i + 1], d = r1 - r0;
            const double* q0 = q + (size_t)i * kMieQ;
            const double* q1 = q0 + kMieQ;
            const double w0 = q0[4] * r0 * r0, w1 = q1[4] * r1 * r1;
            ie += d * (w1 * q1[0] + w0 * q0[0]) / 2.0;
            is += d * (w1 * q1[1] + w0 * q0[1]) / 2.0;
            ig += d * (w1 * q1[1] * q1[3] + w0 * q0[1] * q0[3]) / 2.0;
            in += d * (q1[4] + q0[4]) / 2.0;
        }
        o[0] = is / ie; o[1] = ig / is; o[2] = SOSRT_PI * ie / in;
        return;
    }
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= ntab) return;
    double acc = 0;
    for (int c = 0; c < nchunk; ++c) acc += part[((size_t)s * nchunk + c) * ntab + j];
    p[(size_t)s * ntab + j] = acc;
}

}  // namespace

void launch_epilogue(hipStream_t s, const Grid& g, const double* w, int B, const double* tau, const double* I,
                     const ColDesc* desc, int beam_norm, const double* z_profile, const EpilogueOut& out) {
    hipLaunchKernelGGL(k_epilogue, dim3(B), dim3(256), (size_t)2 * g.L * sizeof(double), s, g, w, B, tau, I, desc, beam_norm,
                       z_profile, out);
}

void launch_azimuth_accumulate(hipStream_t s, const Grid& g, int B, int m, const double* Im, int nlev, const int* levels,
                               int nphi_out, const double* phi, double* out) {
    hipLaunchKernelGGL(k_azimuth_accumulate, dim3(B * nlev), dim3(256), 0, s, g.L, g.D, m, Im, nlev, levels, nphi_out, phi, out);
}

void launch_view_azimuth_accumulate(hipStream_t s, size_t n, int m, const double* val, int nphi_out, const double* phi, double* out) {
    hipLaunchKernelGGL(k_view_azimuth_accumulate, dim3((unsigned)((n * nphi_out + 255) / 256)), dim3(256), 0, s, n, m, val, nphi_out,
                       phi, out);
}

void launch_azimuth_synthesize(hipStream_t s, const Grid& g, int B, int M, const double* I0, const double* Im, int nlev,
                               const int* levels, int nphi_out, const double* phi, double* out) {
    hipLaunchKernelGGL(k_azimuth_synthesize, dim3(B * nlev), dim3(256), 0, s, B, g.L, g.D, M, I0, Im, nlev, levels, nphi_out, phi, out);
}

void launch_mie_coefficients(hipStream_t s, int nlanes, int R, int n_cap, const double* x, const int* nmax, const int* nstart,
                             const double* m_re, const double* m_im, const double* radii, const double* r_m, const double* sig,
                             double* ab, double* qw) {
    hipLaunchKernelGGL(k_mie_coefficients, dim3((nlanes + 63) / 64), dim3(64), 0, s, nlanes, R, n_cap, x, nmax, nstart, m_re,
                       m_im, radii, r_m, sig, ab, qw);
}

void launch_mie_angles(hipStream_t s, int S, int R, int ntab, int n_cap, const double* mu, const double* ab, const int* nmax,
                       const double* tn, const double* qw, double* part) {
    hipLaunchKernelGGL(k_mie_angles, dim3((ntab + 255) / 256, mie_chunks(R), S), dim3(256), 0, s, R, ntab, n_cap, mu, ab, nmax,
                       tn, qw, part);
}

void launch_mie_integrate(hipStream_t s, int S, int R, int ntab, const double* part, const double* radii, const double* qw,
                          double* p, double* bulk) {
    hipLaunchKernelGGL(k_mie_integrate, dim3((ntab + 255) / 256 + 1, S), dim3(256), 0, s, R, ntab, mie_chunks(R), part, radii,
                       qw, p, bulk);
}

}  // namespace sosrt
