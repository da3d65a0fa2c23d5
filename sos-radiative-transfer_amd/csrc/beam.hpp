// Pseudo-spherical direct beam (include/sosrt.h): launchers of beam.hip.  A stage beside the solve: the
// kernels read the columns' scalars and zone tables as sosrt_set_columns* uploaded them (ColScalars) and write their outputs only.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace sosrt {

constexpr int kBeamMaxL = 2048;    // four rows of L doubles in LDS (the first-order kernel): 64 KiB

// sigma [B][L]: slant optical depth of the beam through spherical shells; z [L] km, strictly descending; mu0 [B]
void launch_beam_slant(hipStream_t s, int L, int B, const double* tau, const double* z, double earth_radius, const double* mu0,
                       double* sigma);
// I1 [B][L][D]: the layer-by-layer first order on the beam path sigma [B][L]; p0r_zones > 0: P0r is [B][p0r_zones][D]
void launch_first_order_beam(hipStream_t s, const Grid& g, int B, ColScalars sc, const double* tau, const double* sigma,
                             const double* P0a, const double* P0r, int p0r_zones, double* I1);
// launch_epilogue with the beam terms on the path sigma
void launch_epilogue_beam(hipStream_t s, const Grid& g, const double* w, int B, ColScalars sc, const double* tau,
                          const double* sigma, const double* I, int beam_norm, const double* z_profile, const EpilogueOut& out);

}  // namespace sosrt
