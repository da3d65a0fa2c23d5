// Per-level weights at view lanes, gfx950: the first term of the view radiance of a column whose rows carry
// the weights of sosrt_set_row_weights_dev -- what k_first_order_profile and k_emission_profile (profile.hip)
// are to the grid, at view cosines off it.
//
//   k_view_first_order_profile  k_view_first_order_beam (beam_view.hip) with A and Rz of a ROW: the zone's omega times the
//                               row's weight.  One workgroup of 64 lanes per column, one lane per view pair.
//   k_emission_view_profile     k_emission_view (emission.hip) with the emission coefficient of a ROW.  One workgroup of 64
//                               lanes per column, one lane per view cosine: eps_t belongs to the column, so it is formed once
//                               per row and workgroup in LDS, beside tau and the Planck profile.
//
// Both keep their models' arithmetic: with unit weights every product by a weight is exact, and the expressions are the models'
// own (stage_math.hpp holds what the files share).  The weights of a column are loaded once, coalesced, into LDS (already times
// the zone's omega), outside the lane loop.  The kernels write nothing but their outputs.
#include "profile_view.hpp"
#include "stage_math.hpp"

#include "../../include/sosrt.h"

namespace sosrt {

namespace {

#define SOSRT_PI 3.14159265358979323846

constexpr int kCH = 4;

struct ProfileViewArgs {
    int L, B, V, nset, nlev_all;
    const double* tau;         // [B][L]
    const double* sig;         // [B][L]
    const double* p0a;         // [nset][B][2V]
    const double* p0r;         // [nset][B][2V]
    const double* wa;          // [B][L] the handle's w_atm
    const double* wr;          // [B][L] the handle's w_aer
    double* out;               // [nset][B][nlev_all][2V], offset to the first level of this launch
};

// ------------------------------------------------------------------------------------------
// k_view_first_order_profile: the recurrences, the two exclusions, R, phi, the four coefficient chains and the sorted-level
// cursor of k_view_first_order_beam, with
//   A_t = (omega_atm w_atm,t) f_atm / 4 pi,   Rz_t = (omega_aer w_aer,t) f_aer / 4 pi        (f of row t's zone; clear: f_atm = 1, Rz = 0)
// s_wa[t] = omega_atm w_atm,t and s_wr[t] = omega_aer(zone of t) w_aer,t are formed once per row and workgroup; the fractions
// and 1 / 4 pi stay per zone, multiplied in the model's order.  The zone table is read from LDS, so nothing is indexed
// dynamically in registers.  The three exponentials of a (lane, row) are evaluated once per launch, whatever nset is.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_view_first_order_profile(ProfileViewArgs a, ColScalars sc, ViewMu vm, BeamViewLevels lv) {
    const int L = a.L, V = a.V, V2 = 2 * V;
    const int b = blockIdx.x;
    if (b >= a.B) return;
    extern __shared__ double sm[];
    double* s_tau = sm;             // [L]
    double* s_sig = s_tau + L;      // [L]
    double* s_e0 = s_sig + L;       // [L] F0 e^{-sigma_t}
    double* s_eT = s_e0 + L;        // [L] R e^{-(T - tau_t) / mu0}
    double* s_wa = s_eT + L;        // [L] omega_atm w_atm,t
    double* s_wr = s_wa + L;        // [L] omega_aer of the row's zone times w_aer,t (0 in a clear zone)
    const double* tau = a.tau + (size_t)b * L;
    const double* sig = a.sig + (size_t)b * L;
    const double mu0 = sc.mu0[b], T = sc.T[b], rho = sc.rho[b], wa = sc.alb_atm[b], da = sc.dtau_atm[b];
    const double F0 = SOSRT_PI / mu0;                                        // spec:105
    const double R = F0 * rho * exp(-sig[L - 1] - (T - tau[L - 1]) / mu0);   // the reflected beam at the surface
    const double rmu0 = 1.0 / mu0;
    const int nz = sc.nz[b];
    // the column's zone table, once per workgroup: first rows, kinds and the fractions of spec:149 (1 and 0 in a clear zone)
    __shared__ int zr0[kMaxZones], zmix[kMaxZones];
    __shared__ double zwr[kMaxZones], s_zfa[kMaxZones], s_zfr[kMaxZones];
    if (threadIdx.x < kMaxZones) {
        const int z = threadIdx.x;
        const bool in = z < nz;
        const int mix = in ? sc.zmix[(size_t)b * kMaxZones + z] : 0;
        const double dr = in ? sc.zdtr[(size_t)b * kMaxZones + z] : 0.0;
        zr0[z] = in ? sc.zr0[(size_t)b * kMaxZones + z] : L;
        zmix[z] = mix;
        zwr[z] = in ? sc.zwr[(size_t)b * kMaxZones + z] : 0.0;
        s_zfa[z] = mix ? da / (da + dr) : 1.0;
        s_zfr[z] = mix ? dr / (da + dr) : 0.0;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < L; t += 64) {
        const double tt = tau[t], ss = sig[t];
        const int z = zone_of(zr0, nz, t);
        s_tau[t] = tt;
        s_sig[t] = ss;
        s_e0[t] = F0 * exp(-ss);
        s_eT[t] = R * exp(-(T - tt) / mu0);
        s_wa[t] = wa * a.wa[(size_t)b * L + t];
        s_wr[t] = zmix[z] ? zwr[z] * a.wr[(size_t)b * L + t] : 0.0;
    }
    __syncthreads();
    const int v = threadIdx.x;
    if (v >= V) return;                                      // (no barrier follows)
    const int lo = v, hi = v + V;
    const double ra = 1.0 / vm.s[hi];                        // 1 / mu_v
    const double c4pi = 1.0 / (4 * SOSRT_PI);
    const size_t set_p0 = (size_t)a.B * V2, set_out = (size_t)a.B * a.nlev_all * V2;
    const double* p0a = a.p0a + (size_t)b * V2;
    const double* p0r = a.p0r + (size_t)b * V2;
    double* out = a.out + (size_t)b * a.nlev_all * V2;
    // the lane j's value at the level of place i, for every set
    auto emit = [&](int i, int j, double c0, double c1, double c2, double c3) {
        for (int s = 0; s < a.nset; ++s) {
            const double* pa = p0a + s * set_p0;
            const double* pr = p0r + s * set_p0;
            out[s * set_out + (size_t)i * V2 + j] = (c0 * pa[lo] + c1 * pr[lo]) + (c2 * pa[hi] + c3 * pr[hi]);
        }
    };

    // ---- downward, lane lo ----
    double C0 = 0, C1 = 0, C2 = 0, C3 = 0;                   // D_0 = 0
    int cur = 0, nxt = lv.n > 0 ? lv.t[0] : -1;              // the cursor into the sorted levels and the row it waits for
    auto next_down = [&]() { ++cur; nxt = cur < lv.n ? lv.t[cur] : -1; };
    auto next_up = [&]() { --cur; nxt = cur >= 0 ? lv.t[cur] : -1; };
    for (; nxt == 0; next_down()) emit(lv.idx[cur], lo, 0.0, 0.0, 0.0, 0.0);
    for (int z = 0; z < nz; ++z) {
        const int r0 = zr0[z], r1 = z + 1 < nz ? zr0[z + 1] - 1 : L - 1;
        const double zfa = s_zfa[z], zfr = s_zfr[z];
        const bool top = z == 0;
        for (int tb = max(r0, 1); tb <= r1; tb += kCH) {
            double E[kCH], S0[kCH], S1[kCH], S2[kCH], S3[kCH];
#pragma unroll
            for (int u = 0; u < kCH; ++u) {
                const int t = min(tb + u, r1);
                const double dl = s_tau[t] - s_tau[t - 1], ds = s_sig[t] - s_sig[t - 1];
                const double x = dl * ra;
                const double A = s_wa[t] * zfa * c4pi, Rz = s_wr[t] * zfr * c4pi;
                E[u] = exp(-x);
                const double sd = s_e0[t] * x * phi1(x - ds);
                const double sr = (top || t != r0) ? s_eT[t] * x * phi1(x + dl * rmu0) : 0.0;
                S0[u] = A * sd; S1[u] = Rz * sd; S2[u] = A * sr; S3[u] = Rz * sr;
            }
#pragma unroll
            for (int u = 0; u < kCH; ++u) {
                const int t = tb + u;
                if (t <= r1) {
                    C0 = fma(C0, E[u], S0[u]); C1 = fma(C1, E[u], S1[u]);
                    C2 = fma(C2, E[u], S2[u]); C3 = fma(C3, E[u], S3[u]);
                    for (; nxt == t; next_down()) emit(lv.idx[cur], lo, C0, C1, C2, C3);
                }
            }
        }
    }
    // ---- surface and upward, lane hi (its mirror is lo: the lane's own downward value) ----
    C0 *= rho; C1 *= rho; C2 *= rho; C3 *= rho;
    cur = lv.n - 1;
    nxt = cur >= 0 ? lv.t[cur] : -1;
    for (; nxt == L - 1; next_up()) emit(lv.idx[cur], hi, C0, C1, C2, C3);
    for (int z = nz - 1; z >= 0; --z) {
        const int r0 = zr0[z], r1 = z + 1 < nz ? zr0[z + 1] - 1 : L - 1;
        const double zfa = s_zfa[z], zfr = s_zfr[z];
        const bool bottom = z == nz - 1;
        for (int tb = min(r1, L - 2); tb >= r0; tb -= kCH) {
            double E[kCH], S0[kCH], S1[kCH], S2[kCH], S3[kCH];
#pragma unroll
            for (int u = 0; u < kCH; ++u) {
                const int t = max(tb - u, r0);
                const double dl = s_tau[t + 1] - s_tau[t], ds = s_sig[t + 1] - s_sig[t];
                const double x = dl * ra;
                const double A = s_wa[t] * zfa * c4pi, Rz = s_wr[t] * zfr * c4pi;
                E[u] = exp(-x);
                const double sd = s_e0[t] * x * phi1(x + ds);
                const double sr = (bottom || t != r1) ? s_eT[t] * x * phi1(x - dl * rmu0) : 0.0;
                S0[u] = A * sr; S1[u] = Rz * sr; S2[u] = A * sd; S3[u] = Rz * sd;
            }
#pragma unroll
            for (int u = 0; u < kCH; ++u) {
                const int t = tb - u;
                if (t >= r0) {
                    C0 = fma(C0, E[u], S0[u]); C1 = fma(C1, E[u], S1[u]);
                    C2 = fma(C2, E[u], S2[u]); C3 = fma(C3, E[u], S3[u]);
                    for (; nxt == t; next_up()) emit(lv.idx[cur], hi, C0, C1, C2, C3);
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// k_emission_view_profile: the sweeps and the ground value of k_emission_view at a = mu_view[v], with the emission coefficient
// of a ROW (stage_math.hpp, row_eps: the expression of k_emission_profile).  The layer between rows t-1 and t takes eps_t in
// BOTH sweeps, as there; with eps a row's, the zones are no loop of the sweeps any more: rows 1 .. L-1 in chunks of kCH, the
// exponential and the source term of a row ahead of the chain.  The requested levels arrive sorted by row; a cursor walks them
// with the sweep.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_emission_view_profile(int B, int V, int L, int nlev_all, ColScalars sc, int surface,
                                                              const double* __restrict__ tau_all, const double* __restrict__ pl_all,
                                                              const double* __restrict__ bs_all, const double* __restrict__ es_all,
                                                              const double* __restrict__ wa_all, const double* __restrict__ wr_all,
                                                              double* __restrict__ out_all, ViewMu vm, BeamViewLevels lv) {
    const int b = blockIdx.x;
    if (b >= B) return;                                      // (uniform over the workgroup)
    extern __shared__ double sm[];
    double* s_tau = sm;             // [L]
    double* s_b = s_tau + L;        // [L]
    double* s_eps = s_b + L;        // [L] emission coefficient of the row
    {
        const double* tau = tau_all + (size_t)b * L;
        const double* pl = pl_all + (size_t)b * L;
        const double wa = sc.alb_atm[b], da = sc.dtau_atm[b];
        const int nz = sc.nz[b];
        const int* zr0 = sc.zr0 + (size_t)b * kMaxZones;
        for (int t = threadIdx.x; t < L; t += 64) {
            s_tau[t] = tau[t];
            s_b[t] = pl[t];
            const int z = zone_of(zr0, nz, t);
            const double wat = wa * wa_all[(size_t)b * L + t];
            s_eps[t] = row_eps(sc, b, z, wat, da, wr_all, (size_t)b * L + t);
        }
    }
    __syncthreads();
    const int v = threadIdx.x;
    if (v >= V) return;                                      // (no barrier follows)
    const int V2 = 2 * V;
    const double rmu = 1.0 / vm.s[V + v];
    const double rho = sc.rho[b];
    double* __restrict__ out = out_all + (size_t)b * nlev_all * V2;
    int cur = 0, nxt = lv.n > 0 ? lv.t[0] : -1;              // the cursor into the sorted levels and the row it waits for
    auto next_down = [&]() { ++cur; nxt = cur < lv.n ? lv.t[cur] : -1; };
    auto next_up = [&]() { --cur; nxt = cur >= 0 ? lv.t[cur] : -1; };
    // ---- downward, lane -mu ----
    double Dv = 0;
    for (; nxt == 0; next_down()) out[(size_t)lv.idx[cur] * V2 + v] = 0.0;
    for (int tb = 1; tb <= L - 1; tb += kCH) {
        double E[kCH], S[kCH];
#pragma unroll
        for (int u = 0; u < kCH; ++u) {
            const int t = min(tb + u, L - 1);
            const double x = (s_tau[t] - s_tau[t - 1]) * rmu;
            const double bc = s_b[t], bp = s_b[t - 1], eps = s_eps[t];
            double w0, w1;
            E[u] = exp(-x);
            linear_weights(x, E[u], w0, w1);
            S[u] = eps * (w0 * bc + w1 * bp);
        }
#pragma unroll
        for (int u = 0; u < kCH; ++u) {
            const int t = tb + u;
            if (t <= L - 1) {
                Dv = fma(Dv, E[u], S[u]);
                for (; nxt == t; next_down()) out[(size_t)lv.idx[cur] * V2 + v] = Dv;
            }
        }
    }
    // ---- ground and upward, lane +mu ----
    double Uv = (surface == SOSRT_SURFACE_SPECULAR ? rho * Dv : 0.0) + (es_all ? es_all[b] : 1.0 - rho) * bs_all[b];
    cur = lv.n - 1;
    nxt = cur >= 0 ? lv.t[cur] : -1;
    for (; nxt == L - 1; next_up()) out[(size_t)lv.idx[cur] * V2 + V + v] = Uv;
    for (int tb = L - 1; tb >= 1; tb -= kCH) {               // tb: the row the sweep leaves; it arrives at tb - 1
        double E[kCH], S[kCH];
#pragma unroll
        for (int u = 0; u < kCH; ++u) {
            const int t1 = max(tb - u, 1);
            const double x = (s_tau[t1] - s_tau[t1 - 1]) * rmu;
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
                for (; nxt == t1 - 1; next_up()) out[(size_t)lv.idx[cur] * V2 + V + v] = Uv;
            }
        }
    }
}

}  // namespace

void launch_view_first_order_profile(hipStream_t s, int L, int B, int V, int nset, int nlev_all, ColScalars sc, const double* tau,
                                     const double* sigma, const double* p0a, const double* p0r, const double* w_atm,
                                     const double* w_aer, const ViewMu& mu, const BeamViewLevels& lv, double* out) {
    ProfileViewArgs a{L, B, V, nset, nlev_all, tau, sigma, p0a, p0r, w_atm, w_aer, out};
    hipLaunchKernelGGL(k_view_first_order_profile, dim3((unsigned)B), dim3(64), (size_t)6 * L * sizeof(double), s, a, sc, mu, lv);
}

void launch_emission_view_profile(hipStream_t s, int B, int V, int L, int nlev_all, ColScalars sc, int surface, const double* tau,
                                  const double* planck, const double* planck_surface, const double* emissivity, const double* w_atm,
                                  const double* w_aer, const ViewMu& mu, const BeamViewLevels& lv, double* out) {
    hipLaunchKernelGGL(k_emission_view_profile, dim3((unsigned)B), dim3(64), (size_t)3 * L * sizeof(double), s, B, V, L, nlev_all, sc,
                       surface, tau, planck, planck_surface, emissivity, w_atm, w_aer, out, mu, lv);
}

}  // namespace sosrt
