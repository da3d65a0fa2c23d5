// Thermal emission, gfx950: the radiation the layers and the ground emit, as the zeroth-order field the
// order loop scatters and transports (sosrt_solve_dev, d_I1_in).
//
//   k_emission           the emitted field on the grid's directions: one workgroup per column, one lane per direction pair; a lane
//                        runs the downward recurrence of direction N-1-i, takes the ground value of its mirror direction N+i
//                        (the Lambertian grounds: the column's flux sum through LDS) and runs the upward recurrence.
//   k_emission_view      the same sweeps at view cosines off the grid: one lane per (column, view cosine), the requested levels.
//   k_epilogue_emission  k_epilogue (epilogue.hip) with both beam terms absent.
//
// The kernels read the columns as sosrt_set_columns* uploaded them (ColScalars: scalars and zone tables) and write nothing but
// their outputs.
#include "emission.hpp"
#include "stage_math.hpp"

#include "../../include/sosrt.h"

namespace sosrt {

namespace {

// emission coefficient of zone z of column b: 1 - omega_atm in a clear zone, 1 - (omega_atm f_atm + omega_aer f_aer) in an
// aerosol zone, f of spec:149
__device__ __forceinline__ double zone_eps(const ColScalars& sc, int b, int z) {
    const double wa = sc.alb_atm[b];
    if (!sc.zmix[(size_t)b * kMaxZones + z]) return 1.0 - wa;
    const double da = sc.dtau_atm[b], dr = sc.zdtr[(size_t)b * kMaxZones + z], wr = sc.zwr[(size_t)b * kMaxZones + z];
    return 1.0 - (wa * (da / (da + dr)) + wr * (dr / (da + dr)));
}

// ------------------------------------------------------------------------------------------
// k_emission
// With a = |mu|, Delta the optical thickness of a layer, E = e^{-Delta / a}, b_t the Planck radiance at level t and eps_t the
// emission coefficient of row t's zone (the layer between rows t-1 and t takes eps_t in BOTH sweeps):
//   downward  D_0 = 0,  D_t = D_{t-1} E + eps_t (w0 b_t + w1 b_{t-1})
//   ground    U_{L-1} = boundary(D_{L-1}) + e_s b_s      (boundary: the order loop's rule for the handle's surface)
//   upward    U_t = U_{t+1} E + eps_{t+1} (w0 b_t + w1 b_{t+1})
//   mu = 0    eps_t b_t
// E and the source term of a row do not depend on the recurrence: kCH rows are evaluated together, and the dependent chain is
// one fused multiply-add per row.  The zones are the outer loop: a zone's eps is a scalar of the loop, no table is indexed.
// ------------------------------------------------------------------------------------------
constexpr int kCH = 4;

__global__ __launch_bounds__(1024) void k_emission(Grid g, int B, ColScalars sc, int surface, const double* __restrict__ tau_all,
                                                   const double* __restrict__ pl_all, const double* __restrict__ bs_all,
                                                   const double* __restrict__ es_all, double* __restrict__ I0_all) {
    const int L = g.L, N = g.N, D = g.D;
    const int b = blockIdx.x, i = threadIdx.x;
    if (b >= B) return;                                      // (uniform over the workgroup)
    extern __shared__ double sm[];
    double* s_tau = sm;             // [L]
    double* s_b = s_tau + L;        // [L]
    double* s_sfc = s_b + L;        // [N] the downward surface row (Lambertian grounds)
    double* s_red = s_sfc + N;      // [16]
    const double* tau = tau_all + (size_t)b * L;
    const double* pl = pl_all + (size_t)b * L;
    for (int t = i; t < L; t += blockDim.x) {
        s_tau[t] = tau[t];
        s_b[t] = pl[t];
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
    const int nz = sc.nz[b];
    const int* zr0 = sc.zr0 + (size_t)b * kMaxZones;

    // ---- downward, direction md; the node lane writes eps_t b_t to both nodes of a row ----
    double Dv = 0;
    for (int z = 0; z < nz; ++z) {
        const int r0 = zr0[z], r1 = z + 1 < nz ? zr0[z + 1] - 1 : L - 1;
        const double eps = zone_eps(sc, b, z);
        if (z == 0 && valid) {
            I0[md] = node ? eps * s_b[0] : 0.0;              // D_0 = 0
            if (node) I0[mup] = eps * s_b[0];
        }
        for (int tb = max(r0, 1); tb <= r1; tb += kCH) {
            double E[kCH], S[kCH], V[kCH];
#pragma unroll
            for (int u = 0; u < kCH; ++u) {
                const int t = min(tb + u, r1);
                const double x = (s_tau[t] - s_tau[t - 1]) * rad;
                const double bc = s_b[t], bp = s_b[t - 1];
                double w0, w1;
                E[u] = exp(-x);
                linear_weights(x, E[u], w0, w1);
                S[u] = eps * (w0 * bc + w1 * bp);
                V[u] = eps * bc;
            }
#pragma unroll
            for (int u = 0; u < kCH; ++u) {
                const int t = tb + u;
                if (t <= r1) {
                    Dv = fma(Dv, E[u], S[u]);
                    if (valid) {
                        I0[(size_t)t * D + md] = node ? V[u] : Dv;
                        if (node) I0[(size_t)t * D + mup] = V[u];
                    }
                }
            }
        }
    }
    // ---- ground ----
    double Bv = 0;
    if (surface == SOSRT_SURFACE_SPECULAR) {
        Bv = rho * Dv;                                       // the mirror lane: the lane's own downward value
    } else if (surface == SOSRT_SURFACE_LAMBERTIAN || surface == SOSRT_SURFACE_LAMBERTIAN_README) {
        // -+ 2 rho trapz(D[rev] mu[rev], mu[rev]), rev = N-2 .. 0: the trapezoid of the order loop's boundary (descending
        // abscissae, the mu = 0 node left out), one interval per lane, summed over the column's waves through LDS
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
    for (int z = nz - 1; z >= 0; --z) {
        const int r0 = zr0[z], r1 = z + 1 < nz ? zr0[z + 1] - 1 : L - 1;
        const double eps = zone_eps(sc, b, z);
        const int lo = max(r0, 1);
        for (int tb = r1; tb >= lo; tb -= kCH) {             // tb: the row the sweep leaves; it arrives at tb - 1
            double E[kCH], S[kCH];
#pragma unroll
            for (int u = 0; u < kCH; ++u) {
                const int t1 = max(tb - u, lo);
                const double x = (s_tau[t1] - s_tau[t1 - 1]) * rau;
                const double bc = s_b[t1 - 1], bp = s_b[t1];
                double w0, w1;
                E[u] = exp(-x);
                linear_weights(x, E[u], w0, w1);
                S[u] = eps * (w0 * bc + w1 * bp);
            }
#pragma unroll
            for (int u = 0; u < kCH; ++u) {
                const int t1 = tb - u;
                if (t1 >= lo) {
                    Uv = fma(Uv, E[u], S[u]);
                    if (valid && !node) I0[(size_t)(t1 - 1) * D + mup] = Uv;
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// k_emission_view: the sweeps of k_emission at a = mu_view[v].  One lane per (column, v): the downward sweep of -mu, the ground
// value (specular: rho times the lane's own downward value; no surface: 0; plus e_s b_s), the upward sweep of +mu; the requested
// levels are written, nothing else.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_emission_view(int B, int V, int L, int nlev_all, ColScalars sc, int surface,
                                                      const double* __restrict__ tau_all, const double* __restrict__ pl_all,
                                                      const double* __restrict__ bs_all, const double* __restrict__ es_all,
                                                      double* __restrict__ out_all, ViewMu vm, ViewLevels lv) {
    const int gid = blockIdx.x * 64 + threadIdx.x;
    if (gid >= B * V) return;
    const int V2 = 2 * V;
    const int b = gid / V, v = gid - b * V;
    const double rmu = 1.0 / vm.s[V + v];
    const double* __restrict__ tau = tau_all + (size_t)b * L;
    const double* __restrict__ pl = pl_all + (size_t)b * L;
    double* __restrict__ out = out_all + (size_t)b * nlev_all * V2;
    auto emit = [&](int t, int j, double val) {
        for (int k = 0; k < lv.n; ++k)
            if (lv.t[k] == t) out[(size_t)k * V2 + j] = val;
    };
    const int nz = sc.nz[b];
    const int* zr0 = sc.zr0 + (size_t)b * kMaxZones;
    const double rho = sc.rho[b];
    // ---- downward, lane -mu ----
    double Dv = 0;
    emit(0, v, 0.0);
    for (int z = 0; z < nz; ++z) {
        const int r0 = zr0[z], r1 = z + 1 < nz ? zr0[z + 1] - 1 : L - 1;
        const double eps = zone_eps(sc, b, z);
        double tp = tau[max(r0, 1) - 1], bp = pl[max(r0, 1) - 1];
        for (int t = max(r0, 1); t <= r1; ++t) {
            const double tc = tau[t], bc = pl[t];
            const double x = (tc - tp) * rmu, E = exp(-x);
            double w0, w1;
            linear_weights(x, E, w0, w1);
            Dv = fma(Dv, E, eps * (w0 * bc + w1 * bp));
            emit(t, v, Dv);
            tp = tc; bp = bc;
        }
    }
    // ---- ground and upward, lane +mu ----
    double Uv = (surface == SOSRT_SURFACE_SPECULAR ? rho * Dv : 0.0) + (es_all ? es_all[b] : 1.0 - rho) * bs_all[b];
    emit(L - 1, V + v, Uv);
    for (int z = nz - 1; z >= 0; --z) {
        const int r0 = zr0[z], r1 = z + 1 < nz ? zr0[z + 1] - 1 : L - 1;
        const double eps = zone_eps(sc, b, z);
        const int lo = max(r0, 1);
        double tp = tau[r1], bp = pl[r1];
        for (int t1 = r1; t1 >= lo; --t1) {
            const double tc = tau[t1 - 1], bc = pl[t1 - 1];
            const double x = (tp - tc) * rmu, E = exp(-x);
            double w0, w1;
            linear_weights(x, E, w0, w1);
            Uv = fma(Uv, E, eps * (w0 * bc + w1 * bp));
            emit(t1 - 1, V + v, Uv);
            tp = tc; bp = bc;
        }
    }
}

// ------------------------------------------------------------------------------------------
// k_epilogue_emission: k_epilogue of epilogue.hip, the same arithmetic, without the two beam terms: an emitting atmosphere has
// no direct beam.  One workgroup per column.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_epilogue_emission(Grid g, const double* __restrict__ w_all, int B, ColScalars sc,
                                                           const double* __restrict__ I_all, const double* __restrict__ z_profile,
                                                           EpilogueOut out) {
    const int b = blockIdx.x;
    if (b >= B) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    const int L = g.L, N = g.N, D = g.D;
    extern __shared__ double s_flux[];                       // [2 L]: flux_down + flux_up; heating rate
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
            const size_t o = (size_t)b * L + t;
            if (out.flux_down) out.flux_down[o] = sd;
            if (out.flux_up) out.flux_up[o] = su;
            if (out.diffusivity) out.diffusivity[o] = -(sd + su) / den;
            s_flux[t] = sd + su;
            if (t == 0 && out.net_toa) out.net_toa[b] = -sd - su;
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

void launch_emission(hipStream_t s, const Grid& g, int B, ColScalars sc, int surface, const double* tau, const double* planck,
                     const double* planck_surface, const double* emissivity, double* I0) {
    const int threads = (g.N + 63) / 64 * 64;
    const size_t shm = ((size_t)2 * g.L + g.N + 16) * sizeof(double);
    hipLaunchKernelGGL(k_emission, dim3((unsigned)B), dim3(threads), shm, s, g, B, sc, surface, tau, planck, planck_surface,
                       emissivity, I0);
}

void launch_emission_view(hipStream_t s, int B, int V, int L, int nlev_all, ColScalars sc, int surface, const double* tau,
                          const double* planck, const double* planck_surface, const double* emissivity, const ViewMu& mu,
                          const ViewLevels& lv, double* out) {
    hipLaunchKernelGGL(k_emission_view, dim3((B * V + 63) / 64), dim3(64), 0, s, B, V, L, nlev_all, sc, surface, tau, planck,
                       planck_surface, emissivity, out, mu, lv);
}

void launch_epilogue_emission(hipStream_t s, const Grid& g, const double* w, int B, ColScalars sc, const double* tau,
                              const double* I, const double* z_profile, const EpilogueOut& out) {
    (void)tau;                                               // (no beam term reads the optical depths)
    hipLaunchKernelGGL(k_epilogue_emission, dim3(B), dim3(256), (size_t)2 * g.L * sizeof(double), s, g, w, B, sc, I, z_profile, out);
}

}  // namespace sosrt
