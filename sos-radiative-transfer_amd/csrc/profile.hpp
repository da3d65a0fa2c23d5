// Per-level weights on the source function (include/sosrt.h): launchers of profile.hip.  The weights are the
// handle's copies [B][L] of sosrt_set_row_weights_dev; the stage kernels read the columns' scalars and zone tables as
// sosrt_set_columns* uploaded them (ColScalars) and write their outputs only.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace sosrt {

constexpr int kProfileMaxL = 1024;    // six rows of L doubles in LDS (the first-order kernel): 48 KiB

// dst_a / dst_r [n]: the caller's weights, or ones where a source is null or ends (n_src elements are the caller's)
void launch_row_weights_copy(hipStream_t s, size_t n, size_t n_src, const double* src_a, const double* src_r, double* dst_a,
                             double* dst_r);
// rowcoef_a[b][t] *= w_atm[b][t], rowcoef_r[b][t] *= w_aer[b][t]: behind launch_prepare while weights are set
void launch_row_weights_apply(hipStream_t s, size_t n, const double* w_atm, const double* w_aer, double* rowcoef_a, double* rowcoef_r);
// I1 [B][L][D]: launch_first_order_beam (beam.hpp) with the weights in q, row by row
void launch_first_order_profile(hipStream_t s, const Grid& g, int B, ColScalars sc, const double* tau, const double* sigma,
                                const double* P0a, const double* P0r, int p0r_zones, const double* w_atm, const double* w_aer,
                                double* I1);
// I0 [B][L][D]: launch_emission (emission.hpp) with the weights in the emission coefficient, row by row
void launch_emission_profile(hipStream_t s, const Grid& g, int B, ColScalars sc, int surface, const double* tau, const double* planck,
                             const double* planck_surface, const double* emissivity, const double* w_atm, const double* w_aer,
                             double* I0);

}  // namespace sosrt
