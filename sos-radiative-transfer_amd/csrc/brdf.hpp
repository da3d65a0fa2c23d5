// BRDF ground (include/sosrt.h): launchers of brdf.hip.  Stages beside the solve: the kernels read the grid,
// the columns' mu0 as sosrt_set_columns* uploaded it (ColScalars) and their arguments, and write their outputs only.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace sosrt {

struct BrdfParams {
    int kind;                          // SOSRT_BRDF_*
    double p[3];                       // RPV: rho0, k, Theta
};

// R [N-1][N-1], element (j, i) at j (N-1) + i: 2 w_j |mu_j| rho_bar(mu[N+1+i], |mu_j|)
void launch_brdf_operator(hipStream_t s, const Grid& g, BrdfParams bp, int nphi, double* R);
// r0 [B][N-1]: rho_bar(mu[N+1+i], mu0[b])
void launch_brdf_beam(hipStream_t s, const Grid& g, int B, BrdfParams bp, int nphi, const double* mu0, double* r0);
// Fourier modes m_first .. m_first + m_count - 1 in azimuth, rho^m = (1 / pi) int_0^pi rho cos(m phi) dphi in
// place of rho_bar: R [m_count][N-1][N-1], mode m as (-1)^m R^m where sign_odd; r0 [m_count][B][N-1].  Mode 0: the bits of the two above.
void launch_brdf_operator_modes(hipStream_t s, const Grid& g, BrdfParams bp, int nphi, int m_first, int m_count, int sign_odd,
                                double* R);
void launch_brdf_beam_modes(hipStream_t s, const Grid& g, int B, BrdfParams bp, int nphi, int m_first, int m_count, const double* mu0,
                            double* r0);
// S [B][N-1] = scale (R I[L-1][0 .. N-2] + r0 exp(-tau[L-1] / mu0)); r0, scale nullable
void launch_ground_source(hipStream_t s, const Grid& g, int B, ColScalars sc, const double* I, const double* tau, const double* R,
                          const double* r0, const double* scale, double* S);
// G [B][L][D]: the unscattered field of S with the mu -> 0+ blend on every row; status [B] nullable
void launch_ground_first_order(hipStream_t s, const Grid& g, int B, const double* tau, const double* S, double* G, int* status);
// total += Ik; ratio [B]
void launch_bounce_accumulate(hipStream_t s, const Grid& g, int B, const double* Ik, double* total, double* ratio);
// The ground's term at view lanes; vm.s[0 .. V-1] are the view cosines.  Rows [m_count][N-1][V] = 2 w_j |mu_j|
// rho^m(mu_view_v, |mu_j|) ((-1)^m with sign_odd), beam rows [m_count][B][V] = rho^m(mu_view_v, mu0_b): at a node the bits of the
// two mode builders above.  Beam rows at azimuths [nphi_out][B][V] = rho(mu_view_v, mu0_b, phi_q).
void launch_brdf_view_rows_modes(hipStream_t s, const Grid& g, const ViewMu& vm, int V, BrdfParams bp, int nphi, int m_first,
                                 int m_count, int sign_odd, double* R);
void launch_brdf_view_beam_modes(hipStream_t s, int B, const ViewMu& vm, int V, BrdfParams bp, int nphi, int m_first, int m_count,
                                 const double* mu0, double* r0);
void launch_brdf_view_beam_azimuth(hipStream_t s, int B, const ViewMu& vm, int V, BrdfParams bp, const double* mu0, int nphi_out,
                                   const double* phi, double* out);
// out [B][nlev_all][2V] (offset to the first level of lv): lanes V + v (+)= S exp(-(tau[L-1] - tau[t]) / mu_view_v), S [B][V] =
// scale (Rv I[L-1][0 .. N-2] + r0v exp(-tau[L-1] / mu0)); lanes v = +0 when writing.  I and Rv, r0v, scale, S_out nullable.
void launch_view_ground(hipStream_t s, const Grid& g, int B, int V, const ViewMu& vm, ColScalars sc, const double* I,
                        const double* tau, const double* Rv, const double* r0v, const double* scale, int nlev_all,
                        const ViewLevels& lv, int accumulate, double* S_out, double* out);

}  // namespace sosrt
