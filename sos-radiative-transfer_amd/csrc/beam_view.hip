// Pseudo-spherical direct beam at view lanes, gfx950: the first order layer by layer on a beam path sigma
// that is an INPUT, at view cosines off the direction grid -- the recurrences of k_first_order_beam (beam.hip, DESIGN section
// 17) with the direction's |mu_m| replaced by the lane's view cosine.
//
//   k_view_first_order_beam  one lane per (column, view pair v): the lane runs the downward recurrence of the lane -mu_v,
//                            reflects it at the surface into its own mirror +mu_v and runs the upward one.
//
// A lane's value is linear in the four phase values (p0_atm[lo], p0_aer[lo], p0_atm[hi], p0_aer[hi]) of its two signed lanes
// (lo = v, hi = v + V), with coefficients that depend on the geometry only.  The lane carries the four coefficient recurrences
// instead of the value, so the exponentials of a (lane, row) are evaluated once per launch whatever nset is; at a requested
// level it writes the nset values from the sets' four numbers.
//
// The kernel reads the columns as sosrt_set_columns* uploaded them (ColScalars) and writes nothing but its output.
#include "beam_view.hpp"

#include "../../include/sosrt.h"

namespace sosrt {

namespace {

#define SOSRT_PI 3.14159265358979323846

// phi(y) = (1 - e^{-y}) / y, phi(0) = 1 (beam.hip): exact where the lane's attenuation and the beam's cancel, so a view cosine
// equal to mu0 needs no limit branch
__device__ __forceinline__ double phi1(double y) { return y == 0.0 ? 1.0 : -expm1(-y) / y; }

constexpr int kCH = 4;

struct BeamViewArgs {
    int L, B, V, nset, nlev_all;
    const double* tau;         // [B][L]
    const double* sig;         // [B][L]
    const double* p0a;         // [nset][B][2V]
    const double* p0r;         // [nset][B][2V]
    double* out;               // [nset][B][nlev_all][2V], offset to the first level of this launch
};

// ------------------------------------------------------------------------------------------
// With a = mu_v, Delta the optical thickness of a layer, x = Delta / a, E = e^{-x}, dsig the beam's slant thickness of the layer,
// q = A p0_atm + Rz p0_aer of the zone (A = w_atm f_atm / (4 pi), Rz = w_aer f_aer / (4 pi); clear zone: f_atm = 1, Rz = 0):
//   downward  D_t = D_{t-1} E + q_t[lo] F0 e^{-sigma_t} x phi(x - dsig)
//                             + [t not the first row of a zone below the top one] q_t[hi] R e^{-(T - tau_t) / mu0} x phi(x + Delta / mu0)
//   surface   U_{L-1} = rho D_{L-1}
//   upward    U_t = U_{t+1} E + q_t[hi] F0 e^{-sigma_t} x phi(x + dsig)
//                             + [t not the last row of a zone above the bottom one] q_t[lo] R e^{-(T - tau_t) / mu0} x phi(x - Delta / mu0)
// carried as C = (coefficient of p0_atm[lo], of p0_aer[lo], of p0_atm[hi], of p0_aer[hi]): four chains of one fused multiply-add
// per row.  A row's (E, Sd, Sr) hold its three exponentials and do not depend on the chains: kCH rows are evaluated together,
// ahead of them.  The two beam attenuations of a row do not depend on the lane: once per row and workgroup, in LDS.  The
// zones are the outer loop, so no table is indexed dynamically in registers.  The requested levels arrive sorted by row; a
// cursor walks them with the sweep, the row it waits for in a register.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_view_first_order_beam(BeamViewArgs a, ColScalars sc, ViewMu vm, BeamViewLevels lv) {
    const int L = a.L, V = a.V, V2 = 2 * V;
    const int b = blockIdx.x;
    if (b >= a.B) return;
    extern __shared__ double sm[];
    double* s_tau = sm;             // [L]
    double* s_sig = s_tau + L;      // [L]
    double* s_e0 = s_sig + L;       // [L] F0 e^{-sigma_t}
    double* s_eT = s_e0 + L;        // [L] R e^{-(T - tau_t) / mu0}
    const double* tau = a.tau + (size_t)b * L;
    const double* sig = a.sig + (size_t)b * L;
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
    const int v = threadIdx.x;
    if (v >= V) return;                                      // (no barrier follows)
    const int lo = v, hi = v + V;
    const double ra = 1.0 / vm.s[hi];                        // 1 / mu_v
    const double c4pi = 1.0 / (4 * SOSRT_PI);
    const int nz = sc.nz[b];
    const int* zr0 = sc.zr0 + (size_t)b * kMaxZones;
    const int* zmix = sc.zmix + (size_t)b * kMaxZones;
    const double* zwr = sc.zwr + (size_t)b * kMaxZones;
    const double* zdtr = sc.zdtr + (size_t)b * kMaxZones;
    // q of zone z = A p0_atm + Rz p0_aer (spec:149)
    auto zone_w = [&](int z, double& A, double& Rz) {
        A = wa * c4pi;
        Rz = 0.0;
        if (zmix[z]) {
            const double dr = zdtr[z], wr = zwr[z];
            A = wa * (da / (da + dr)) * c4pi;
            Rz = wr * (dr / (da + dr)) * c4pi;
        }
    };
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
    // the cursor into the sorted levels and the row it waits for (-1: none left), kept in a register: the chains compare rows
    // against it and read the kernel arguments only when a level is written
    int cur = 0, nxt = lv.n > 0 ? lv.t[0] : -1;
    auto next_down = [&]() { ++cur; nxt = cur < lv.n ? lv.t[cur] : -1; };
    auto next_up = [&]() { --cur; nxt = cur >= 0 ? lv.t[cur] : -1; };
    for (; nxt == 0; next_down()) emit(lv.idx[cur], lo, 0.0, 0.0, 0.0, 0.0);
    for (int z = 0; z < nz; ++z) {
        const int r0 = zr0[z], r1 = z + 1 < nz ? zr0[z + 1] - 1 : L - 1;
        double A, Rz;
        zone_w(z, A, Rz);
        const bool top = z == 0;
        for (int tb = max(r0, 1); tb <= r1; tb += kCH) {
            double E[kCH], S0[kCH], S1[kCH], S2[kCH], S3[kCH];
#pragma unroll
            for (int u = 0; u < kCH; ++u) {
                const int t = min(tb + u, r1);
                const double dl = s_tau[t] - s_tau[t - 1], ds = s_sig[t] - s_sig[t - 1];
                const double x = dl * ra;
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
        double A, Rz;
        zone_w(z, A, Rz);
        const bool bottom = z == nz - 1;
        for (int tb = min(r1, L - 2); tb >= r0; tb -= kCH) {
            double E[kCH], S0[kCH], S1[kCH], S2[kCH], S3[kCH];
#pragma unroll
            for (int u = 0; u < kCH; ++u) {
                const int t = max(tb - u, r0);
                const double dl = s_tau[t + 1] - s_tau[t], ds = s_sig[t + 1] - s_sig[t];
                const double x = dl * ra;
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

}  // namespace

void launch_view_first_order_beam(hipStream_t s, int L, int B, int V, int nset, int nlev_all, ColScalars sc, const double* tau,
                                  const double* sigma, const double* p0a, const double* p0r, const ViewMu& mu,
                                  const BeamViewLevels& lv, double* out) {
    BeamViewArgs a{L, B, V, nset, nlev_all, tau, sigma, p0a, p0r, out};
    hipLaunchKernelGGL(k_view_first_order_beam, dim3((unsigned)B), dim3(64), (size_t)4 * L * sizeof(double), s, a, sc, mu, lv);
}

}  // namespace sosrt
