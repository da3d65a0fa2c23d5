// Delta-M scaling of a tabulated phase function: the Legendre moments of the table's piecewise-linear
// interpolant, and the table of the series truncated at order Lambda.  Kernels in deltam.hip, entry points in api_deltam.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace sosrt {

constexpr int kDeltaMMaxTab = 65536;     // SOSRT_DELTAM_MAX_NTAB
constexpr int kDeltaMMaxOrder = 128;     // SOSRT_DELTAM_MAX_LMAX
constexpr int kDeltaMBlock = 256;        // threads of a workgroup: one table interval each (moments), one abscissa each (table)

// workgroups a table's intervals are cut into: a function of ntab alone, so the order of every sum is
inline int deltam_chunks(int ntab) { return (ntab - 1 + kDeltaMBlock - 1) / kDeltaMBlock; }
// doubles of workspace the moments of S tables need: the chunks' partial sums [S][chunks][lmax + 1]
inline size_t deltam_moments_workspace(int S, int ntab, int lmax) { return (size_t)S * deltam_chunks(ntab) * (lmax + 1); }

// chi [S][lmax + 1] (and norm [S], nullable) of the tables tab_p [S][ntab] on tab_mu [ntab] (nullptr: the uniform abscissa
// i * step - 1 with the last point 1, step = 2 / (ntab - 1)); part: deltam_moments_workspace doubles
void launch_phase_moments(hipStream_t s, int S, const double* tab_mu, const double* tab_p, int ntab, int lmax, double* part,
                          double* chi, double* norm);
// tab_out [S][ntab] = sum_{l < order} (2l + 1) (chi_l - f) / (1 - f) P_l(x_i), f = chi[order], and f_out [S]; coef: S * order
// doubles of workspace
void launch_phase_delta_m(hipStream_t s, int S, const double* chi, int lmax, int order, const double* tab_mu, int ntab,
                          double* coef, double* tab_out, double* f_out);

}  // namespace sosrt
