// BRDF ground (include/sosrt.h): launchers of brdf.hip.  Stages beside the solve: the kernels read the grid,
// the columns' mu0 as sosrt_set_columns* uploaded it (ColScalars) and their arguments, and write their outputs only.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace sosrt {

struct BrdfParams {
    int kind;                          // SOSRT_BRDF_*
    double p[3];                       // RPV: rho0, k, Theta; the Ross-Li kernels: mu_floor; Cox-Munk: sigma2, n, shadow
};

// The Fourier modes m_first .. m_first + m_count - 1 in azimuth of the named BRDF, rho^m(a, b) = (1 / pi) int_0^pi rho cos(m phi)
// dphi on nphi trapezoid nodes (mode 0: the azimuth mean rho_bar), for every pair of a first direction a and a second b.  a: the
// view cosines vm.s[0 .. V-1], or with V = 0 the grid's upward nodes mu[N+1+i].  b: the columns' mu0 [B], or
// with mu0 = nullptr the grid's downward nodes |mu_j| with the flux quadrature folded in.  The four layouts of out:
//   V = 0, mu0 = nullptr   the operator   [m_count][N-1][N-1], element (j, i) = 2 w_j |mu_j| rho^m(mu[N+1+i], |mu_j|)
//   V = 0, mu0             the beam rows  [m_count][B][N-1] = rho^m(mu[N+1+i], mu0[b])
//   V > 0, mu0 = nullptr   the view rows  [m_count][N-1][V], element (j, v) = 2 w_j |mu_j| rho^m(mu_view_v, |mu_j|)
//   V > 0, mu0             the view beam rows [m_count][B][V] = rho^m(mu_view_v, mu0[b])
// sign_odd (the grid's b only): mode m as (-1)^m of it.  A mode's bits are the same however many modes a call takes and from which
// it starts, and at a view cosine equal to a node those of the node.
void launch_brdf_pairs(hipStream_t s, const Grid& g, const ViewMu& vm, int V, int B, BrdfParams bp, int nphi, int m_first,
                       int m_count, int sign_odd, const double* mu0, double* out);
// S [B][N-1] = scale (R I[L-1][0 .. N-2] + r0 exp(-tau[L-1] / mu0)); r0, scale nullable
void launch_ground_source(hipStream_t s, const Grid& g, int B, ColScalars sc, const double* I, const double* tau, const double* R,
                          const double* r0, const double* scale, double* S);
// S [B][N-1] = sum_k weight[b][k] (R_k I[L-1][0 .. N-2] + r0_k[b] exp(-tau[L-1] / mu0)), k ascending in fused multiply-adds from +0;
// R [K][N-1][N-1], r0 [K][B][N-1] (nullable), weight [B][K].  K = 1: the bits of launch_ground_source with scale = weight.
void launch_ground_source_terms(hipStream_t s, const Grid& g, int B, int K, ColScalars sc, const double* I, const double* tau,
                                const double* R, const double* r0, const double* weight, double* S);
// launch_view_ground with the same sum over K terms: Rv [K][N-1][V], r0v [K][B][V], weight [B][K]
void launch_view_ground_terms(hipStream_t s, const Grid& g, int B, int K, int V, const ViewMu& vm, ColScalars sc, const double* I,
                              const double* tau, const double* Rv, const double* r0v, const double* weight, int nlev_all,
                              const ViewLevels& lv, int accumulate, double* S_out, double* out);
// G [B][L][D]: the unscattered field of S with the mu -> 0+ blend on every row; status [B] nullable
void launch_ground_first_order(hipStream_t s, const Grid& g, int B, const double* tau, const double* S, double* G, int* status);
// total += Ik; ratio [B]
void launch_bounce_accumulate(hipStream_t s, const Grid& g, int B, const double* Ik, double* total, double* ratio);
// Beam rows at azimuths [nphi_out][B][V] = rho(mu_view_v, mu0_b, phi_q), no quadrature.
void launch_brdf_view_beam_azimuth(hipStream_t s, int B, const ViewMu& vm, int V, BrdfParams bp, const double* mu0, int nphi_out,
                                   const double* phi, double* out);
// out [B][nlev_all][2V] (offset to the first level of lv): lanes V + v (+)= S exp(-(tau[L-1] - tau[t]) / mu_view_v), S [B][V] =
// scale (Rv I[L-1][0 .. N-2] + r0v exp(-tau[L-1] / mu0)); lanes v = +0 when writing.  I and Rv, r0v, scale, S_out nullable.
void launch_view_ground(hipStream_t s, const Grid& g, int B, int V, const ViewMu& vm, ColScalars sc, const double* I,
                        const double* tau, const double* Rv, const double* r0v, const double* scale, int nlev_all,
                        const ViewLevels& lv, int accumulate, double* S_out, double* out);

}  // namespace sosrt
